"""The launch plan of the multi-wave MH kernels (fugue_amd/csrc/fg_mh_mw_plan.h) against tests/golden/mh_mw_plans.json.

MH results are bit-identical whatever the plan (LDS size, W, the mode bits, which wave gets which record, what the run-time compiler
is asked to generate), so only this test sees a change of the plan.  The fixture was recorded from the launchers of the commit its
header names, before the plan was a set of functions of its own: their planning lines, copied behind stand-in engine structs and run
on these cases with the switches in the environment.  `python tests/test_mh_mw_plan_cpu.py --record` rewrites the expected values
from the current code after a deliberate change; review the diff of the fixture.

The cases are small synthetic record lists (`model`), not the benchmark models; REACHED counts, per item the plan can decide, the
cases that reach it.
"""
import json
import math
import os
import shutil
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "mh_mw_plans.json")
SWITCHES = ("pipe", "exp", "split", "prio", "prio2", "stagger", "catu", "jit", "gen_min", "gen_all", "nseg", "nseg_ns", "ctl16", "bake", "jit_any", "jit_sums",
            "sums_form")      # FG_MH_PIPE, _EXP, _SPLIT, _PRIO, _PRIO2, _STAGGER, _CATU, FG_JIT, FG_MH_GEN_MIN, _GEN_ALL, _NSEG, _NSEG_NS, _CTL16, _BAKE, _JIT_ANY, _JIT_SUMS, _SUMS_FORM
DEFAULTS = dict(recs="f*3,o*4", acc=None, sites="f*3", C=65536, n_simd=1024, mw=0, ov=0, nins=1000, slots_extra=0, pool_pad=0, xcat=0, kinds=None, gen=None,
                **{k: None for k in SWITCHES})       # None: the switch is unset; acc: a program without a score stream (its sites from `sites`)
F64, BOOL, USIZE = 0, 1, 3
G_POW2, G_LIN, G_GEN, G_NSEL, G_CATC = 2, 256, 1024, 1 << 27, 1 << 28
GENERAL = ("g", "n", "i", "l", "b", "zc")        # record tokens that are class 5 by construction


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def expand(spec):
    out = []
    for part in spec.split(","):
        name, _, n = part.partition("*")
        out += [name] * int(n or 1)
    return out


def model(c):
    """A case's program as fg_program.cpp would lay it out.  Record tokens: f an f64 site's Normal prior (class 4), s a prior whose mean
    is a site (2), o an observation of a site's mean (3), g / b a general record / a bool site's prior, n a Normal whose sigma is no power
    of two, i both operands site + immediate, l a linear predictor (all class 5); cuK / cnK / czK / cyK a Categorical site with a constant
    table of K entries: uniform / not uniform / equal logs but a zero probability past the first / in the first entry (class 1); zs / zc an
    observation against an option list of sites / with one constant entry (class 0 / 5).  Prior terms take rows 0 .. n_pri, then the rest."""
    toks = expand(c["recs"]) if c["acc"] is None else []
    sites, pool, recs = [], [], []                    # sites: (vtype, cat base, K); recs: [xi, mi, flags, prior, ximm, mimm]
    Z = -1                                            # the always-zero slot (the last one), patched below
    for t in (expand(c["sites"]) if c["acc"] is not None else []):
        sites.append(({"f": F64, "b": BOOL, "c": USIZE}[t], -1, -1))
    n_f64 = lambda: max(1, sum(1 for s in sites if s[0] == F64))
    for k, t in enumerate(toks):
        if t == "f":
            sites.append((F64, -1, -1)); recs.append([len(sites) - 1, Z, G_POW2, 1, 0, 0])
        elif t == "s":
            sites.append((F64, -1, -1)); recs.append([len(sites) - 1, 0, G_POW2, 1, 0, 0])
        elif t == "o":
            recs.append([Z, k % n_f64(), G_POW2, 0, bits(1.5), 0])
        elif t == "g":
            recs.append([Z, 0, G_GEN | (12 << 16), 0, bits(0.5), 0])
        elif t == "n":
            recs.append([Z, 0, 0, 0, bits(0.5), 0])
        elif t == "i":
            recs.append([0, 0, G_POW2, 0, bits(1.0), 0])
        elif t == "l":
            recs.append([Z, Z, G_LIN | G_POW2, 0, bits(1.0), 0])
        elif t == "b":
            sites.append((BOOL, -1, -1)); recs.append([len(sites) - 1, Z, G_GEN, 1, 0, 0])
        elif t[0] == "c":
            K = int(t[2:])
            p = [1.0 / K] * K
            lnp = [math.log(1.0 / K)] * K
            if t[1] == "n":
                p = [0.5] + [0.5 / (K - 1)] * (K - 1); lnp = [math.log(v) for v in p]
            elif t[1] == "z":
                p[1] = 0.0
            elif t[1] == "y":
                p[0] = 0.0
            sites.append((USIZE, len(pool), K))
            recs.append([len(sites) - 1, Z, G_CATC, 1, 0, len(pool) | (K << 32)])
            pool += [bits(v) for v in p + lnp]
        elif t in ("zs", "zc"):
            idx = [j for j, s in enumerate(sites) if s[0] == USIZE]
            recs.append([Z, idx[k % len(idx)] if idx else 0, G_NSEL | G_POW2, 0, bits(0.25), len(pool) | (2 << 32)])
            pool += [0, bits(0.0), (1 | (1 << 32)) if t == "zc" else 1, bits(2.0 if t == "zc" else 0.0)]
        else:
            raise ValueError(t)
    if c["xcat"]:                                     # a Categorical site with a table and no record
        sites.append((USIZE, len(pool), 2)); pool += [bits(0.5)] * 2 + [bits(math.log(0.5))] * 2
    pool += [bits(1.0)] * c["pool_pad"]
    n_slots = len(sites) + c["slots_extra"] + 1
    n_pri = sum(r[3] for r in recs)
    rows, a, b = [], 0, n_pri
    for r in recs:
        r[0] = n_slots - 1 if r[0] == Z else r[0]; r[1] = n_slots - 1 if r[1] == Z else r[1]
        rows.append(a if r[3] else b); a += r[3]; b += 1 - r[3]
    kinds = c["kinds"] if c["kinds"] is not None else (0 if set(toks) <= {"f", "s", "o", "n", "i"} else 1 if set(toks) <= {"f", "s", "o", "n", "i", "l"} else 2)
    gen = c["gen"] if c["gen"] is not None else int(any(t in ("g", "b") for t in toks))
    acc = [int(t) for t in expand(c["acc"])] if c["acc"] is not None else None
    return dict(toks=toks, sites=sites, pool=pool, recs=recs, rows=rows, n_slots=n_slots, n_pri=n_pri, kinds=kinds, gen=gen, acc=acc, n_general=sum(t in GENERAL for t in toks))


def case_line(over):
    c = dict(DEFAULTS, **over)
    m = model(c)
    head = [int(m["acc"] is not None), c["C"], c["n_simd"], m["n_slots"], len(m["sites"]), c["mw"], c["ov"], m["kinds"], m["gen"], m["n_pri"], c["nins"]]
    head += ["u" if c[k] is None else c[k] for k in SWITCHES]
    head += [s[0] for s in m["sites"]] + [v for s in m["sites"] for v in s[1:]] + [len(m["pool"])] + m["pool"]
    if m["acc"] is not None:
        head += [len(m["acc"])] + m["acc"]
    else:
        head += [len(m["recs"]) + 2] + [v for r, row in zip(m["recs"], m["rows"]) for v in (r[0], r[1], r[2], row, r[4], r[5])] + [0] * 12
    return " ".join(str(x) for x in head)


def parse_plan(line):
    """A driver output line -> {field: [integers]}, the two kernel names (library instantiation | generated unit) as they are."""
    body, _, name = line.partition(" name=")
    plan = {k: [int(x) for x in v.split(",") if x] for k, v in (t.split("=") for t in body.split())}
    if name:
        plan["name"] = name.split("|")
    return plan


def runs(v):
    """A list of integers without loss as plain integers, [a, n] = a, a + 1, ... (n of them) and [a, -n] = a, n times."""
    out, i = [], 0
    while i < len(v):
        n = {step: next(k for k in range(1, len(v) - i + 1) if i + k == len(v) or v[i + k] != v[i] + step * k) for step in (0, 1)}
        step = 0 if n[0] >= n[1] else 1
        if n[step] >= 3:
            out.append([v[i], n[step] if step else -n[step]]); i += n[step]
        else:
            out.append(v[i]); i += 1
    return out


def unruns(r):
    return [y for x in r for y in ([x] if isinstance(x, int) else list(range(x[0], x[0] + x[1])) if x[1] > 0 else [x[0]] * -x[1])]


def pack(plan, names):
    """The fixture's form of a plan: every list as `runs`, the table sites' (slot, K) pairs as two lists, the names by index."""
    out = {k: runs(v) for k, v in plan.items() if k not in ("name", "catu")}
    if "catu" in plan:
        out["catu"] = [runs(plan["catu"][0::2]), runs(plan["catu"][1::2])]
    if "name" in plan:
        if plan["name"] not in names:
            names.append(plan["name"])
        out["name"] = names.index(plan["name"])
    assert unpack(out, names) == plan
    return out


def unpack(out, names):
    plan = {k: unruns(v) for k, v in out.items() if k not in ("name", "catu")}
    if "catu" in out:
        plan["catu"] = [v for pair in zip(unruns(out["catu"][0]), unruns(out["catu"][1])) for v in pair]
    if "name" in out:
        plan["name"] = names[out["name"]]
    return plan


def build_driver(out_dir):
    exe = os.path.join(str(out_dir), "mh_plan_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "mh_plan_driver.cpp"), "-o", exe], check=True)
    return exe


def run_plans(exe, cases, work_dir):
    path = os.path.join(str(work_dir), "cases.txt")
    with open(path, "w") as f:
        f.write("".join(case_line(c[0]) + "\n" for c in cases))
    lines = subprocess.run([exe, path], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(cases)
    return [parse_plan(ln.strip()) for ln in lines]


SHAPE = ("lds", "W", "exp_mask", "split", "pool_n", "pipe", "resident", "tiles")
SPEC = ("rk", "split", "n_pri", "n_fac", "no_stream", "pipe", "nseg", "ctl16", "sum_pri", "sum_lik", "bake", "bake_rows", "sums_form")


def reached(c, m, p):
    """The names of the items of the plan's rules that this case reaches (c: the case, m: its model, p: its plan)."""
    out = set()
    stream = m["acc"] is None
    if p["rc"] != [0]:
        out.add("lds over 160 KB: unsupported")
    if stream:
        n_cats = sum(t[0] == "c" for t in m["toks"])
        if p["n_cu"][0]:
            out.add("tail accepted, equal constants" if p["catu_same"][0] else "tail accepted, different constants")
            assert p["n_cu"][0] == n_cats >= 4 and len(p["catu"]) == 2 * n_cats and len(p["catu_c"]) % 8 == 0 and len(p["catu_c"]) >= n_cats + 16
        elif n_cats:
            cats = [t for t in m["toks"] if t[0] == "c"]
            last = all(t[0] == "c" for t in [t for t, r in zip(m["toks"], m["recs"]) if r[3]][-n_cats:])
            why = ("FG_MH_CATU=0" if c["catu"] == 0 else "fewer than 4 tables" if n_cats < 4 else "a table site without a record" if c["xcat"] else "not the last rows" if not last
                   else "a non-uniform table" if any(t[1] == "n" for t in cats) else "a zero probability" if any(t[1] == "z" for t in cats)
                   else "a zero first probability" if any(t[1] == "y" for t in cats) else None)
            assert why, "the tail of this case should have been accepted"
            out.add("tail refused: " + why)
    if p["rc"] != [0]:
        return out
    s = dict(zip(SHAPE, p["shape"]))
    n_rows = p["cls_off"][6] if stream else len(m["acc"])
    if s["lds"] == 160 * 1024:
        out.add("lds exactly 160 KB")
    if c["split"] is None:
        out.add("split by rule, %s 64 rows" % ("under" if n_rows < 64 else "from"))
        assert s["split"] == int(n_rows >= 64)
        if n_rows in (63, 64):
            out.add("split rule at %d rows" % n_rows)
    else:
        out.add("FG_MH_SPLIT=%d" % (c["split"] != 0))
    out.add("resident %s" % min(s["resident"], 3))
    for bit in (32, 64, 128, 512, 1024, 2048, 4096, 16384):
        out.add("bit %d %s" % (bit, "on" if s["exp_mask"] & bit else "off"))
    if c["prio"] == 0 and s["resident"] >= 2:
        out.add("FG_MH_PRIO=0 takes bit 64")
    if c["stagger"] == 0 and s["resident"] >= 3:
        out.add("FG_MH_STAGGER=0 takes bit 128")
    if s["pipe"] and not s["exp_mask"] & 2048:
        out.add("bit 2048 off: " + ("overrides" if c["ov"] and all(v[0] == F64 for v in m["sites"]) else "a site that is not f64"))
    out.add("W=%d %s" % (s["W"], "forced" if c["mw"] > 0 else "by the growth rule"))
    if c["mw"] == 0 and s["resident"] == 1:          # (one tile per CU: only the row count stops the growth)
        out.add("growth: %d rows, %s -> W=%d" % (n_rows, "stream" if stream else "no stream", s["W"]))
    if stream and m["kinds"] and m["pool"]:
        size = len(m["pool"]) * 8
        base = s["lds"] - s["pool_n"] * 8
        out.add("pool staged" if s["pool_n"] else "pool refused: over 24 KB" if size > 24 * 1024 else "pool refused: the tile would pass 160 KB" if base + size > 160 * 1024
                else "pool refused: it would cost a resident tile")
        if not s["pool_n"] and size <= 24 * 1024 and base + size <= 160 * 1024:
            assert (160 * 1024) // base != (160 * 1024) // (base + size)
    if stream:
        for cl in range(6):
            if p["cls_off"][cl + 1] > p["cls_off"][cl]:
                out.add("class %d" % cl)
        if "zc" in m["toks"]:
            k = m["toks"].index("zc")
            assert p["cls_off"][5] <= p["order"].index(k) < p["cls_off"][6]
            out.add("an option list with a constant entry is class 5")
        uneven = any((p["cls_off"][cl + 1] - p["cls_off"][cl]) % s["W"] for cl in range(6))
        if uneven:
            out.add("deal: " + ("even shares" if not (s["pipe"] and s["W"] >= 3) else "proposer %s share, %s" % ("half a" if s["W"] < 8 else "no", "split" if s["split"] else "no split")))
        out.add("key %d %d %d" % tuple(p["key"]))
    if not p["tried"][0]:
        out.add("no unit: " + ("FG_JIT=0" if c["jit"] == 0 else "FG_MH_EXP" if c["exp"] is not None else "the program's size" if c["nins"] > 200000 else "statements outside the three sums"))
        return out
    if c["nins"] == 200000:
        out.add("200 000 instructions: still a unit")
    if not p["unit"][0]:
        assert 8 * m["n_general"] < len(m["toks"])
        out.add("no unit: 8 n_gen < n_s")
        return out
    sp = dict(zip(SPEC, p["spec"]))
    if not stream:
        out.add("no-stream spec, n_fac %s" % ("> 0" if sp["n_fac"] else "= 0"))
        out.add("no-stream spec, " + ("FG_MH_NSEG_NS=0" if c["nseg_ns"] == 0 else "one segment per wave"))
        out.add("no-stream bake %s" % ("on" if sp["bake"] else "off"))
        return out
    n_s, n_gen, all_gen = len(m["toks"]), m["n_general"], all(g or (p["n_cu"][0] and t[0] == "c") for g, t in zip(p["generated"], m["toks"]))
    lookups = p["cls_off"][2] > 0
    if c["gen_all"] is not None:
        out.add("FG_MH_GEN_ALL=%d" % (c["gen_all"] != 0))
    elif c["gen_min"] is not None:
        out.add("FG_MH_GEN_MIN %s n_s" % ("over" if c["gen_min"] > n_s else "within"))
    elif not lookups:
        out.add("gen_all by rule")
        assert all_gen
    if (lookups and c["gen_all"] is None) or c["gen_all"] == 0 or (c["gen_all"] is None and (c["gen_min"] or 0) > n_s):      # n_gen is the count of class-5 records
        assert all_gen == (2 * n_gen >= n_s)
        for mul in (2, 8):
            if mul * n_gen >= n_s:
                out.add("%d n_gen >= n_s%s" % (mul, ", exactly" if mul * n_gen == n_s else ""))
            else:
                out.add("%d n_gen < n_s%s" % (mul, ", by one record" if mul * (n_gen + 1) >= n_s else ""))
        if 8 * n_gen < n_s:
            out.add("FG_MH_JIT_ANY")
            assert c["jit_any"]
    if c["nseg"] == 0:
        out.add("FG_MH_NSEG=0")
        assert sp["nseg"] == 0 and not sp["bake"]
    if c["ctl16"] is not None:
        out.add("FG_MH_CTL16 " + ("below 0" if c["ctl16"] < 0 else "over 16" if c["ctl16"] > 16 else "in range"))
        assert sp["ctl16"] == max(0, min(16, c["ctl16"]))
    out.add("FG_MH_BAKE %s: bake %s%s" % ("unset" if c["bake"] is None else c["bake"], "on" if sp["bake"] else "off", "" if sp["bake_rows"] else ", without the row counts"))
    if s["pipe"] and c["bake"] != 0 and c["nseg"] != 0 and all_gen:
        out.add("bake refused under pipe")
        assert not sp["bake"]
    out.add("FG_MH_JIT_SUMS=0" if sp["sum_pri"] < 0 else "sums' row counts")
    if c["sums_form"] is None:
        out.add("sums form %d by rule" % sp["sums_form"])
        assert sp["sums_form"] == (4 if s["resident"] <= 1 else 0)
    else:
        out.add("FG_MH_SUMS_FORM")
    return out


# every item the cases must reach (the issue's list), spelled as `reached` names them
REACHED = """
split rule at 63 rows|split rule at 64 rows|FG_MH_SPLIT=0|FG_MH_SPLIT=1|resident 1|resident 2|resident 3|bit 32 on|bit 64 on|bit 64 off|bit 128 on|bit 128 off|
FG_MH_PRIO=0 takes bit 64|FG_MH_STAGGER=0 takes bit 128|bit 16384 on|bit 16384 off|bit 512 on|bit 512 off|bit 1024 on|bit 1024 off|bit 2048 on|bit 2048 off|bit 4096 on|bit 4096 off|
bit 2048 off: overrides|bit 2048 off: a site that is not f64|
W=2 by the growth rule|W=4 by the growth rule|W=8 by the growth rule|W=16 by the growth rule|W=2 forced|W=4 forced|W=8 forced|W=16 forced|
growth: 7 rows, stream -> W=2|growth: 8 rows, stream -> W=4|growth: 15 rows, stream -> W=4|growth: 16 rows, stream -> W=8|growth: 95 rows, stream -> W=8|growth: 96 rows, stream -> W=16|
growth: 31 rows, no stream -> W=8|growth: 32 rows, no stream -> W=16|
lds exactly 160 KB|lds over 160 KB: unsupported|pool staged|pool refused: over 24 KB|pool refused: it would cost a resident tile|
tail accepted, equal constants|tail accepted, different constants|tail refused: fewer than 4 tables|tail refused: a non-uniform table|tail refused: a zero probability|
tail refused: a zero first probability|tail refused: not the last rows|tail refused: a table site without a record|tail refused: FG_MH_CATU=0|
class 0|class 1|class 2|class 3|class 4|class 5|an option list with a constant entry is class 5|
deal: even shares|deal: proposer half a share, no split|deal: proposer half a share, split|deal: proposer no share, no split|deal: proposer no share, split|
gen_all by rule|FG_MH_GEN_ALL=0|FG_MH_GEN_ALL=1|FG_MH_GEN_MIN over n_s|FG_MH_GEN_MIN within n_s|2 n_gen >= n_s, exactly|2 n_gen < n_s, by one record|8 n_gen >= n_s, exactly|
no unit: 8 n_gen < n_s|FG_MH_JIT_ANY|FG_MH_NSEG=0|FG_MH_CTL16 below 0|FG_MH_CTL16 over 16|FG_MH_CTL16 in range|FG_MH_BAKE 0: bake off|FG_MH_BAKE unset: bake on|
FG_MH_BAKE 2: bake on, without the row counts|bake refused under pipe|FG_MH_JIT_SUMS=0|sums' row counts|sums form 4 by rule|sums form 0 by rule|FG_MH_SUMS_FORM|
no unit: FG_JIT=0|no unit: FG_MH_EXP|no unit: the program's size|200 000 instructions: still a unit|no unit: statements outside the three sums|
no-stream spec, n_fac > 0|no-stream spec, n_fac = 0|no-stream spec, FG_MH_NSEG_NS=0|no-stream spec, one segment per wave|no-stream bake on|no-stream bake off
""".replace("\n", "").split("|")
UNREACHED = {}       # items no case reaches, each with its reason (none)


def test_every_plan_is_the_recorded_one_and_every_rule_is_reached(tmp_path):
    assert shutil.which("g++"), "g++ builds the driver"
    fx = json.load(open(FIXTURE))
    exe = build_driver(tmp_path)
    plans = run_plans(exe, fx["cases"], tmp_path)
    assert len(plans) >= 100
    count = {}
    for case, have in zip(fx["cases"], plans):
        want = unpack(case[1], fx["names"])
        assert sorted(want) == sorted(have), case[0]
        for field in want:
            assert have[field] == want[field], (case[0], field)
        c = dict(DEFAULTS, **case[0])
        for item in reached(c, model(c), have):
            count[item] = count.get(item, 0) + 1
    table = [tuple(int(x) for x in ln.split()) for ln in subprocess.run([exe, "variants"], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert len(table) == len(set(table)) == 12
    want = set(REACHED) | {"key %d %d %d" % k for k in table}
    assert want - set(count) == set(UNREACHED), sorted(want - set(count))


if __name__ == "__main__" and "--record" in sys.argv:
    import tempfile
    fx = json.load(open(FIXTURE))
    with tempfile.TemporaryDirectory() as td:
        names = []
        for case, plan in zip(fx["cases"], run_plans(build_driver(td), fx["cases"], td)):
            case[1] = pack(plan, names)
    fx["names"] = names
    fx["recorded_from"] = subprocess.run(["git", "-C", ROOT, "describe", "--always", "--dirty"], capture_output=True, text=True).stdout.strip()
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(fx[k], separators=(",", ":")) for k in fx if k != "cases") +
                ',\n"cases": [\n' + ",\n".join(json.dumps(c, separators=(",", ":")) for c in fx["cases"]) + "\n]}\n")
