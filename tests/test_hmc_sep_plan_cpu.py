"""The launch plan of k_hmc_sep_steps (fg_hmc_sep_plan, fugue_amd/csrc/fg_hmc_sep_plan.h) against tests/golden/hmc_sep_plans.json.

Results are bit-identical whatever the plan (tile width, W, the wave split, sum4, the priority / stagger flags), so only this test
sees a change of the plan.  The fixture was recorded from the launcher of the commit its header names, before the plan was a function of
its own; `python tests/test_hmc_sep_plan_cpu.py --record` rewrites the expected values from the current code after a deliberate change.
"""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "hmc_sep_plans.json")
DEFAULTS = dict(d=32, C=65536, s="u0obs", g=1, m=0, mw=0, n_simd=1024, gt=0, sep_off=0, res_off=0, fold_off=0, sep_fold=1,
                half=None, dfast=None, sum4=None, prio=None, stagger=None, predraw=None)       # g: FG_GRAD_*; None: the switch is unset
SWITCHES = ("half", "dfast", "sum4", "prio", "stagger", "predraw")    # FG_HMC_SEP_HALF, _DENSE_FAST, _SUM4, _PRIO, _STAGGER, _PREDRAW


def records(shape, d):
    """(n_sep_free, [(off, n)] per coordinate, [trow] per record) of a program of `d` coordinates as fg_program.cpp lays it out:
    a coordinate's prior record, then its observations; prior rows first, then the observation rows in program order."""
    n_free = 2 if shape.endswith("free") else 0
    nrec = {"r1": 1, "r2": 2, "r3": 3, "r4": 4, "u0obs": 2, "nonp2": 2, "r2rev": 2, "r1free": 1, "r2free": 2}.get(shape)
    per = [nrec if nrec else (1 + i % 3 if shape == "mixed" else 2) for i in range(d)]
    flags = [0 if shape == "nonp2" or (shape == "mixp2" and i % 2) else (256 | (512 if shape == "u0obs" else 0)) for i in range(d)]
    n_pri = d + (1 if n_free else 0)                                     # (one of the two free statements is a prior term)
    prior_row = [(d - 1 - i) if shape == "r2rev" else i for i in range(d)]
    coord, trow, off, obs_row = [], [], 0, n_pri
    for i in range(d):
        coord.append((off, per[i] | flags[i]))
        trow.append(prior_row[i])
        for _ in range(per[i] - 1):
            trow.append(obs_row)
            obs_row += 1
        off += per[i]
    return n_free, coord, trow + [0] * 4


def case_line(over):
    c = dict(DEFAULTS, **over)
    n_free, coord, trow = records(c["s"], c["d"])
    n_sstream = len(trow) - 4 + n_free
    head = [c["C"], c["d"], c["n_simd"], n_sstream + 2, n_free, n_sstream, c["g"], c["m"], c["mw"], c["gt"], c["sep_off"], c["res_off"], c["fold_off"], c["sep_fold"]]
    head += ["u" if c[k] is None else c[k] for k in SWITCHES]
    return " ".join(str(x) for x in head + [len(coord)] + [v for q in coord for v in q] + [len(trow)] + trow)


def parse_plan(line):
    """A driver output line -> the plan as a dict of plain values (rc alone when the kernel does not take the launch)."""
    t = line.split(" ", 1 + 5 + 7 + 17 + 2 + 16 + 64)
    if len(t) == 1:
        return {"rc": int(t[0])}
    v = [int(x) for x in t[:-1]]
    return {"rc": v[0], "half": v[1], "tw": v[2], "tiles": v[3], "W": v[4], "lds": v[5], "key": v[6:13], "c": v[13:30], "sum4": v[30], "predraw": v[31],
            "n_own": v[32:48], "own": [v[48 + 4 * w:52 + 4 * w] for w in range(16)], "name": t[-1]}


def pack(plan, names):
    """The fixture's form of a plan: c[0..15] without the repeats of its last value, n_own / own without trailing zeros, the name by index."""
    if plan["rc"] != 0:
        return plan["rc"]
    c = plan["c"][:16]
    while len(c) > 1 and c[-1] == c[-2]:
        c.pop()
    n_own = list(plan["n_own"])
    while n_own and n_own[-1] == 0:
        n_own.pop()
    own = [row[:n] for row, n in zip(plan["own"], n_own)]
    assert unpack([0, 0, 0, 0, 0, 0, c, plan["c"][16], 0, 0, n_own, own, 0], [""])["own"] == plan["own"]     # (nothing but zeros was dropped)
    if plan["name"] not in names:
        names.append(plan["name"])
    return [plan["half"], plan["tw"], plan["tiles"], plan["W"], plan["lds"], plan["key"], c, plan["c"][16], plan["sum4"], plan["predraw"], n_own, own, names.index(plan["name"])]


def unpack(out, names):
    if isinstance(out, int):
        return {"rc": out}
    half, tw, tiles, W, lds, key, c, c16, sum4, predraw, n_own, own, name = out
    return {"rc": 0, "half": half, "tw": tw, "tiles": tiles, "W": W, "lds": lds, "key": key, "c": c + [c[-1]] * (16 - len(c)) + [c16], "sum4": sum4, "predraw": predraw,
            "n_own": n_own + [0] * (16 - len(n_own)), "own": [row + [0] * (4 - len(row)) for row in own] + [[0] * 4] * (16 - len(own)), "name": names[name]}


def build_driver(out_dir):
    exe = os.path.join(str(out_dir), "sep_plan_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "sep_plan_driver.cpp"), "-o", exe], check=True)
    return exe


def run_plans(exe, cases, work_dir):
    path = os.path.join(str(work_dir), "cases.txt")
    with open(path, "w") as f:
        f.write("".join(case_line(c[0]) + "\n" for c in cases))
    lines = subprocess.run([exe, path], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(cases)
    return [parse_plan(ln) for ln in lines]


# table entries no case reaches, each with its reason (none)
UNREACHED = {}


def test_every_plan_is_the_recorded_one_and_every_variant_is_reached(tmp_path):
    assert shutil.which("g++"), "g++ builds the driver"
    fx = json.load(open(FIXTURE))
    exe = build_driver(tmp_path)
    plans = run_plans(exe, fx["cases"], tmp_path)
    assert len(plans) >= 200
    for case, got in zip(fx["cases"], plans):
        assert got == unpack(case[1], fx["names"]), case[0]
    table = [tuple(int(x) for x in ln.split()) for ln in subprocess.run([exe, "variants"], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert len(table) == len(set(table)) == 58
    keys = {tuple(p["key"]) for p in plans if p["rc"] == 0}
    assert keys <= set(table), keys - set(table)
    assert set(table) - keys == set(UNREACHED), sorted(set(table) - keys)


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
