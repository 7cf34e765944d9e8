"""The host side of adaptive_smc ahead of its launches (fugue_amd/csrc/fg_smc_plan.h) against tests/golden/smc_plans.json: the plan of
the rejuvenation sweep (fg_smc_rejuv_plan), the shape of the compiled sweep (fg_smc_jit_rejuv_shape) and the layout of the engine's SMC
arena (fg_smc_arena_layout).

Results do not depend on which rejuvenation kernel runs on which grid, so only this test sees a change of the plan.  The expected values
were recorded from the launchers of the commit the fixture names, before the plan was a function of its own: that commit's expressions,
lifted verbatim into a program outside the repository.  Only the kernels' names are the header's own (that commit had none).
`python tests/test_smc_plan_cpu.py --record` rewrites the expected values from the current code after a deliberate change.
"""
import itertools
import json
import os
import shutil
import subprocess
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "smc_plans.json")
SAN = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g")
FG_E_UNSUPPORTED = -6

# n_slots: where 150 KB / (512 n_slots) crosses 16, 8, 4, 3, 2, 1 and where the global tile begins; S: the compiled sweep's 16 -> 4 tiles per
# block (2 | 3), its 150 KB refusal (300 | 301), the block histogram (320 | 321); N: the tile, the 16-tile block, the population rule
N_SLOTS = (1, 18, 19, 37, 38, 75, 76, 100, 101, 150, 151, 300, 301)
SITES = (1, 2, 3, 75, 76, 300, 301, 320, 321)
PARTICLES = (1, 63, 64, 65, 1023, 1024, 1025, 2 ** 18 - 1, 2 ** 18, 2 ** 20)
SCORES = {-1: (0, 0, 0), 0: (1, 0, 0), 2: (1, 1, 1), 3: (1, 1, 0)}            # score class -> has_sstream, sstream_kinds, sstream_gen
KEEP_ONE_IN = 280                                                            # of the 56 160 combinations below; each with from_run 0 and 1
ARENA_CASES = [(n, s) for n in (1, 2047, 2048, 2049, 2 ** 20) for s in (0, 1, 40, 400)]
ESS2_DOUBLES = 2 * 256 * 8 * 2 + 2 + 2 * 128 // 8 + 2                        # Reducer::ess2_doubles() (fg_smc.hip): sizeof(FgEssBracket) = 128


def rejuv_cases():
    """The cross product of the values above, thinned: one combination in KEEP_ONE_IN by a fixed hash, and every (n_slots, score class)
    once as a batched sweep (the tiles per block are a function of that pair), every (N, jit_state) once on a fast-Normal stream (the
    population rule).  Both callers of every combination are kept (but
    fg_smc_rejuvenate has no sequential mode: no such launch to record)."""
    out = []
    for c in itertools.product(N_SLOTS, SITES, PARTICLES, sorted(SCORES), (-1, 0, 1), (0, 1), (0, 1)):
        if zlib.crc32(repr(c).encode()) % KEEP_ONE_IN == 0 or c[1:3] + c[4:] == (3, 1025, 0, 1, 0) or c[:2] + (c[3],) + c[5:] == (18, 3, 0, 1, 0):
            n_slots, S, N, score, jit_state, d, seq = c
            out += [dict(N=N, S=S, d=d, n_slots=n_slots, score=score, jit_state=jit_state, seq=seq, from_run=fr) for fr in (0, 1) if fr or not seq]
    return out


def case_line(c):
    return "rejuv " + " ".join(str(x) for x in (c["N"], c["S"], c["d"], c["n_slots"], 64) + SCORES[c["score"]] + (c["jit_state"], c["seq"], c["from_run"]))


def parse(line):
    plan, shape, name = line.split(" | ")
    return [int(x) for x in plan.split()], [int(x) for x in shape.split()], name


def build_driver(out_dir, flags=()):
    exe = os.path.join(str(out_dir), "smc_plan_driver" + ("_san" if flags else ""))
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", *flags, os.path.join(ROOT, "tests", "cpp", "smc_plan_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_driver(exe, lines, env=None):
    r = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def all_lines():
    return [case_line(c) for c in rejuv_cases()] + [f"arena {n} {s} {ESS2_DOUBLES}" for n, s in ARENA_CASES]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    assert shutil.which("g++"), "g++ builds the driver"
    return build_driver(tmp_path_factory.mktemp("smc_plan"))


def test_every_rejuvenation_plan_is_the_recorded_one_and_every_rule_is_reached(driver):
    fx = json.load(open(FIXTURE))
    cases = rejuv_cases()
    assert [c[0] for c in fx["rejuv"]] == cases and 300 <= len(cases) <= 1200
    got = [parse(ln) for ln in run_driver(driver, [case_line(c) for c in cases])]
    reached = {k: 0 for k in ("global tile by LDS", "global tile by site count", "compiled unit tried by score", "compiled unit tried by population and jit_state",
                              "compiled unit refused by S", "compiled unit refused by tile size", "the from_run difference", "no coordinate to move", "sequential")}
    wpb_seen = {s: set() for s in SCORES}
    by_in = {}
    for (c, want_plan, want_shape, name), (plan, shape, got_name) in zip(fx["rejuv"], got):
        assert plan == want_plan and shape == want_shape and got_name == (fx["names"][name] if name is not None else "-"), c
        if shape[0] != 0:
            assert shape == [FG_E_UNSUPPORTED]
            reached["compiled unit refused by S" if c["S"] > 320 else "compiled unit refused by tile size"] += 1
        if plan[0] != 0:
            assert plan == [FG_E_UNSUPPORTED] and c["d"] == 0
            reached["no coordinate to move"] += 1
            continue
        _, score, gt, wpb, lds, nblk, threads, tried, k_score, k_gt, k_seq = plan
        assert (k_score, k_gt, k_seq) == (score, gt, c["seq"]) and score == c["score"]
        assert lds <= 150 * 1024 and threads <= 1024 and (c["seq"] or nblk * threads >= c["N"]), c      # a block within the hardware's limits, a lane per particle
        if gt:
            assert (wpb, lds, threads, tried) == (1, 0, 64, 0)
            reached["global tile by site count" if c["S"] > 320 else "global tile by LDS"] += 1
        if c["seq"]:
            assert (nblk, threads, tried) == (1, 64, 0)
            reached["sequential"] += 1
        elif not gt:
            wpb_seen[score].add(wpb)
        if tried:
            reached["compiled unit tried by score" if score != 0 else "compiled unit tried by population and jit_state"] += 1
        by_in[tuple(sorted(c.items()))] = tried
    for c in cases:
        if c["from_run"] == 1 and c["d"] > 0 and not c["seq"]:
            twin = by_in[tuple(sorted(dict(c, from_run=0).items()))]
            if by_in[tuple(sorted(c.items()))] != twin:
                assert c["score"] == 0 and c["jit_state"] == 1 and c["N"] >= 2 ** 18 and not c["seq"] and twin == 0, c
                reached["the from_run difference"] += 1
    assert all(reached.values()), reached
    # each value of tiles per block, per score class: the kernel's own number, then what 150 KB hold (n_slots 19, 37 | 38, 75 | 76, 100 | 101, 150 | 151)
    assert wpb_seen == {-1: {1}, 2: {4, 3, 2, 1}, 0: {16, 15, 8, 7, 4, 3, 2, 1}, 3: {16, 15, 8, 7, 4, 3, 2, 1}}, wpb_seen
    table = [tuple(int(x) for x in ln.split()) for ln in subprocess.run([driver, "variants"], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert len(table) == len(set(table)) == 8
    for seq in (0, 1):                                        # both tables (k_smc_rejuv, k_smc_rejuv_seq): every entry reached, no key without an entry
        keys = {(p[0][8], p[0][9]) for p in got if p[0][0] == 0 and p[0][10] == seq}
        assert keys == set(table), (seq, keys ^ set(table))


def test_the_arena_is_the_recorded_one_aligned_disjoint_and_the_reset_covers_the_adaptation(driver):
    fx = json.load(open(FIXTURE))
    names = subprocess.run([driver, "regions"], capture_output=True, text=True, check=True).stdout.split()
    assert names == fx["regions"] and len(names) == 22
    assert [tuple(c[0]) for c in fx["arena"]] == ARENA_CASES
    out = run_driver(driver, [f"arena {n} {s} {ESS2_DOUBLES}" for n, s in ARENA_CASES])
    for (case, (total, reset_from, reset_to, offs)), ln in zip(fx["arena"], out):
        v = [int(x) for x in ln.split()]
        bytes_, reset_off, reset_bytes, off, length = v[0], v[1], v[2], v[3::2], v[4::2]
        assert bytes_ == total and off == offs, case                                  # the parent's total, the parent's offsets
        assert all(o % 256 == 0 for o in off) and all(n > 0 for n in length), case
        spans = sorted(zip(off, length))
        assert spans[0][0] == 0 and all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] <= bytes_, case
        at = dict(zip(names, zip(off, length)))
        assert names[3:7] == ["log_scale", "acc", "tot", "st"]                         # carved in this sequence: the reset is one range
        assert reset_off == at["log_scale"][0] == reset_from and reset_off + reset_bytes == at["tot"][0] + at["tot"][1] <= reset_to == at["st"][0], case
        inside = [nm for nm in names if at[nm][0] < reset_off + reset_bytes and reset_off < at[nm][0] + at[nm][1]]
        assert inside == ["log_scale", "acc", "tot"], case


def test_driver_under_address_and_ub_sanitizers(tmp_path):
    """The stand-alone driver built with -fsanitize=address,undefined over the same cases: the same output, and a finding ends the run
    with a non-zero status."""
    assert shutil.which("g++"), "g++ builds the driver"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=24")
    lines = all_lines()
    assert run_driver(build_driver(tmp_path, SAN), lines, env) == run_driver(build_driver(tmp_path), lines)


if __name__ == "__main__" and "--record" in sys.argv:
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        exe = build_driver(td)
        cases, names, rejuv = rejuv_cases(), [], []
        for c, ln in zip(cases, run_driver(exe, [case_line(c) for c in cases])):
            plan, shape, name = parse(ln)
            if name != "-" and name not in names:
                names.append(name)
            rejuv.append([c, plan, shape, names.index(name) if name != "-" else None])
        arena = []
        for case, ln in zip(ARENA_CASES, run_driver(exe, [f"arena {n} {s} {ESS2_DOUBLES}" for n, s in ARENA_CASES])):
            v = [int(x) for x in ln.split()]
            arena.append([list(case), [v[0], v[1], v[3::2][6], v[3::2]]])             # total, the reset's start, the scalars' offset behind it, every offset
        regions = subprocess.run([exe, "regions"], capture_output=True, text=True, check=True).stdout.split()
    fx = {"recorded_from": subprocess.run(["git", "-C", ROOT, "describe", "--always", "--dirty"], capture_output=True, text=True).stdout.strip(),
          "names": names, "regions": regions, "arena": arena, "rejuv": rejuv}
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(fx[k], separators=(",", ":")) for k in ("recorded_from", "names", "regions")) +
                ',\n"arena": [\n' + ",\n".join(json.dumps(c, separators=(",", ":")) for c in arena) + '\n],\n"rejuv": [\n' +
                ",\n".join(json.dumps(c, separators=(",", ":")) for c in rejuv) + "\n]}\n")
