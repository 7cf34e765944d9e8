"""The plans of the wave-split HMC launchers (fugue_amd/csrc/fg_hmc_split_plan.h) against tests/golden/hmc_split_plans.json.

Results are bit-identical whatever the split (waves per tile, which wave owns which task, the one-barrier form, the program in LDS), so
only this test sees a change of a plan.  The fixture was recorded from the launchers' own lines of the commit its header names, before the
plans were functions of their own; `python tests/test_hmc_split_plan_cpu.py --record` rewrites the expected values from the current code
after a deliberate change.  Every rule of the plans must be reached by at least one case (RULES).
"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "hmc_split_plans.json")
DENSE, SPARSE, ANALYTIC = 0, 1, 2                 # FG_GRAD_FD_DENSE, FG_GRAD_FD_SPARSE, FG_GRAD_ANALYTIC (include/fugue_amd.h)
LDS = 160 * 1024
G_X_CONST, G_M_CONST, G_LIN, G_GEN = 32, 64, 256, 1024      # fg_ir.h
U = "u"                                           # a switch that is unset

# sub-programs of a coordinate: (hoisted densities, general densities, fast Normals, plain operations); cost 10 / 16 / 3 / 1 each
FAST, FAST2, GEN1, HEAVY, EMPTY = (0, 0, 1, 0), (0, 0, 2, 0), (0, 1, 0, 2), (2, 12, 0, 5), (0, 0, 0, 0)


def coords(spec, d):
    return [spec[k % len(spec)] for k in range(d)] if isinstance(spec, list) else [spec] * d


def jit_case(d=8, S=20, n_simd=1024, mw=0, tiles0=3, sw0=(U, U, U), tasks=U, tiles=None, sw=None, mode=SPARSE, has_ad=1, sub=FAST):
    """sw0 / sw: (FG_HMC_INTERP_WAVES, FG_HMC_JIT_OCC, FG_JIT_FUSED) when the unit is generated / when its split is prepared."""
    c = dict(kind="jit", d=d, S=S, n_simd=n_simd, mw=mw, tiles0=tiles0, sw0=tuple(sw0), tasks=tasks, tiles=tiles0 if tiles is None else tiles,
             sw=tuple(sw0 if sw is None else sw), mode=mode, has_ad=has_ad, sub=coords(sub, d))
    c["line"] = " ".join(str(x) for x in ["jit", d, S, n_simd, mw, c["tiles0"], *c["sw0"], tasks, c["tiles"], *c["sw"], mode, has_ad] + [v for q in c["sub"] for v in q])
    return c


def mwi_case(d=6, S=12, n_slots=20, mw=0, n_simd=1024, tiles=257, prog_bytes=9600, mode=SPARSE, sw=(U, U, U), tiles2=None, sw2=None, sub=GEN1):
    """sw / sw2: (FG_HMC_INTERP_WAVES, _OCC, _LDSPROG) at an engine's first / a later launch."""
    c = dict(kind="mwi", d=d, S=S, n_slots=n_slots, mw=mw, n_simd=n_simd, tiles=tiles, prog_bytes=prog_bytes, mode=mode, sw=tuple(sw), tiles2=tiles if tiles2 is None else tiles2,
             sw2=tuple(sw if sw2 is None else sw2), sub=coords(sub, d))
    c["line"] = " ".join(str(x) for x in ["mwi", d, S, n_slots, mw, n_simd, tiles, prog_bytes, mode, *c["sw"], c["tiles2"], *c["sw2"]] + [v for q in c["sub"] for v in q])
    return c


def stream_case(d=8, tiles=1024, n_simd=1024, lds_bytes=40960, mw=0, tw=64, gt=0, mode=SPARSE, kinds=0, has_ss=1, recs=None):
    """recs: (coord, flags, maskm, xi, mi) per record, in coordinate order; default: one prior record per coordinate reading itself."""
    recs = [(k, G_M_CONST, 0, k, 0) for k in range(d)] if recs is None else recs
    c = dict(kind="stream", d=d, tiles=tiles, n_simd=n_simd, lds_bytes=lds_bytes, mw=mw, tw=tw, gt=gt, mode=mode, kinds=kinds, has_ss=has_ss, recs=recs)
    c["line"] = " ".join(str(x) for x in ["stream", d, tiles, n_simd, lds_bytes, mw, tw, gt, mode, kinds, has_ss, len(recs)] + [v for r in recs for v in r])
    return c


def chain(d, obs=1, flags=0):
    """A prior record per coordinate and `obs` records that read the coordinate before it as mu (hier-like)."""
    out = []
    for k in range(d):
        out.append((k, G_M_CONST | flags, 0, k, 0))
        out += [(k, G_X_CONST | flags, 0, 0, max(0, k - 1))] * obs
    return out


def all_cases():
    cs = []
    # fg_task_ins_cost: one instruction per opcode class (densities hoisted or not, the fast Normal, transcendental, pow, div / sqrt, a DOT of n terms, the rest)
    for op, opnd1 in [(0, 0), (0 | 512, 0), (16, 0), (16 | 512, 0), (20, 0), (48, 0), (49, 0), (53, 0), (54, 0), (55, 0), (56, 0), (57, 0), (44, 0), (46, 0), (50, 0),
                      (66, 0), (66, 1), (66, 9), (66, 64), (40, 0), (41, 0), (43, 0), (61, 0), (62, 0), (32, 0), (65, 0)]:
        cs.append(dict(kind="cost", line=f"cost {op} {opnd1}"))
    # ---- the compiled unit: generated at tiles0 under sw0, prepared at tiles under sw
    for d in (1, 2, 3, 5, 8, 12):                                           # a CU has at most one tile: W = wcap = min(16, 4 occ, 2 d)
        cs.append(jit_case(d=d))
        cs.append(jit_case(d=d, sw0=(U, 2, U)))
        cs.append(jit_case(d=d, sw0=(U, 3, U), mode=DENSE))
    cs.append(jit_case(d=8, sw0=(U, 7, U)))                                 # (FG_HMC_JIT_OCC outside 2 .. 4 is ignored)
    for d, S, tiles in [(8, 20, 1024), (8, 20, 257), (6, 30, 1024), (8, 20, 768), (8, 60, 1024), (8, 150, 1024), (12, 20, 1024), (9, 20, 8192), (3, 4, 1024), (1, 4, 4096),
                        (8, 250, 1024)]:
        for mode in (SPARSE, DENSE, ANALYTIC):                              # several tiles per CU: target 4 (four resident tiles, <= 16 tasks) or 8
            cs.append(jit_case(d=d, S=S, tiles0=tiles, mode=mode))
    for forced in (1, 2, 5, 8, 16, 40):                                     # forced W: FG_HMC_INTERP_WAVES over FG_HMC_WAVES, clamped to [1, wcap]
        cs.append(jit_case(d=6, tiles0=1024, sw0=(forced, U, U)))
        cs.append(jit_case(d=6, tiles0=1024, mw=forced, mode=DENSE))
    cs.append(jit_case(d=6, tiles0=1024, mw=2, sw0=(4, U, U)))
    cs.append(jit_case(d=10, tiles0=1024, mw=40, sw0=(U, 2, U)))
    # the one-barrier form: the 96-unit span rule, the residency rule, FG_JIT_FUSED
    for sub in (FAST, FAST2, GEN1, [HEAVY, FAST, FAST], [GEN1, FAST, EMPTY], [HEAVY, GEN1]):
        for tiles in (3, 1024):
            cs.append(jit_case(d=8, tiles0=tiles, sub=sub))
            cs.append(jit_case(d=5, tiles0=tiles, sub=sub, mode=ANALYTIC, has_ad=0))
            cs.append(jit_case(d=7, tiles0=tiles, sub=sub, sw0=(U, U, 1)))
            cs.append(jit_case(d=7, tiles0=tiles, sub=sub, sw0=(U, U, 0)))
    for S, d in [(150, 8), (155, 4), (100, 30), (140, 12), (250, 8)]:        # the second copy of the site rows: lds2 beyond 160 KB, or a resident tile lost
        for fused in (U, 1, 0):
            for mode in (SPARSE, DENSE):
                cs.append(jit_case(d=d, S=S, tiles0=1024, sw0=(U, U, fused), mode=mode))
    for d, forced in [(8, 4), (6, 4), (5, 2), (5, 3), (9, 6), (12, 8), (7, 16)]:   # the dense coordinate split: 2 ceil(d / W) = ceil(2 d / W) or not
        cs.append(jit_case(d=d, tiles0=1024, sw0=(forced, U, U), mode=DENSE))
        cs.append(jit_case(d=d, tiles0=1024, sw0=(forced, U, 1), mode=DENSE))
    # generated behind one split, prepared under another: chain counts, switches, FG_JIT_TASKS=0
    for mode in (SPARSE, DENSE, ANALYTIC):
        for sub in (FAST, [HEAVY, FAST, GEN1]):
            cs.append(jit_case(d=8, tiles0=3, tiles=1024, mode=mode, sub=sub))
            cs.append(jit_case(d=8, tiles0=1024, tiles=257, mode=mode, sub=sub))
            cs.append(jit_case(d=8, tiles0=1024, tiles=3, mode=mode, sub=sub))
            cs.append(jit_case(d=8, tiles0=1024, tasks=0, mode=mode, sub=sub))
            cs.append(jit_case(d=8, tiles0=1024, tasks=1, mode=mode, sub=sub))
            cs.append(jit_case(d=8, tiles0=1024, sw0=(U, U, 0), sw=(U, U, U), mode=mode, sub=sub))
            cs.append(jit_case(d=8, tiles0=1024, sw0=(U, U, U), sw=(U, U, 0), mode=mode, sub=sub))
            cs.append(jit_case(d=8, tiles0=1024, sw0=(U, U, U), sw=(2, U, U), mode=mode, sub=sub))
            cs.append(jit_case(d=8, tiles0=1024, sw0=(8, U, U), sw=(U, 2, U), mode=mode, sub=sub))
    # ---- the interpreter kernel: the split at the first launch, the shape at every launch
    for d in (2, 3, 6, 12):
        for mode in (SPARSE, DENSE):
            cs.append(mwi_case(d=d, mode=mode, sub=[GEN1, HEAVY, FAST]))
    for forced in (1, 2, 3, 8, 12, 16, 40):
        cs.append(mwi_case(d=12, sw=(forced, U, U)))
        cs.append(mwi_case(d=12, mw=forced, sw=(U, 2, U)))
    cs.append(mwi_case(d=12, mw=4, sw=(8, U, U)))
    for n_slots, S in [(60, 12), (90, 12), (130, 12), (170, 12), (140, 100), (330, 300), (300, 20)]:   # private rows: the doubling stopped by the LDS, the shrink loop
        cs.append(mwi_case(d=6, S=S, n_slots=n_slots))
        cs.append(mwi_case(d=6, S=S, n_slots=n_slots, sw=(8, U, U)))
    for tiles in (3, 256, 257, 1024):                                       # the program in LDS: 80 KB with two tiles on a CU, 160 KB for a CU's only tile
        for prog_bytes in (960, 50016, 76800, 120000, 160032):
            cs.append(mwi_case(tiles=tiles, prog_bytes=prog_bytes))
    for ldsprog in (0, 1, 2):
        for prog_bytes in (960, 120000, 163200):
            cs.append(mwi_case(prog_bytes=prog_bytes, sw=(U, U, ldsprog)))
    for occ in (1, 2, 3, 4, 8):
        cs.append(mwi_case(d=12, sw=(U, occ, U)))
        cs.append(mwi_case(d=12, sw=(16, occ, U)))
    cs.append(mwi_case(d=12, sw=(U, U, U), sw2=(2, 2, 0), tiles2=3))        # a later launch: W stays, occ and the program's place follow the switches
    cs.append(mwi_case(d=12, sw=(16, U, U), sw2=(U, 2, U), tiles=3, tiles2=1024, prog_bytes=100032))
    cs.append(mwi_case(d=12, sw=(2, 2, 0), sw2=(U, U, U)))
    # ---- the gradient-stream kernel
    for mw in (1, 2, 5, 16, 40):
        cs.append(stream_case(mw=mw, recs=chain(8)))
    for d, tiles, lds_bytes in [(8, 1024, 40960), (8, 257, 40960), (8, 3, 40960), (32, 3, 61440), (64, 3, 90000), (3, 3, 20000), (20, 8192, 30000), (12, 512, 163840), (40, 1024, 81920)]:
        cs.append(stream_case(d=d, tiles=tiles, lds_bytes=lds_bytes, recs=chain(d)))      # resident W < 16 until a wave would own fewer than four coordinates
        cs.append(stream_case(d=d, tiles=tiles, lds_bytes=lds_bytes))                      # independent coordinates: separable
        cs.append(stream_case(d=d, tiles=tiles, lds_bytes=lds_bytes, mode=DENSE))          # dense stream: even cuts, no records
        cs.append(stream_case(d=d, tiles=tiles, lds_bytes=lds_bytes, mode=ANALYTIC, recs=chain(d, obs=2)))
    lin = [(k, G_M_CONST, 0, k, 0) for k in range(16)]
    cs.append(stream_case(d=16, tiles=3, recs=lin))
    for at, terms in [(0, 40), (3, 40), (15, 40), (8, 6), (8, 200)]:          # a linear predictor costs 1 + terms / 2: its coordinate's cut moves
        recs = list(lin)
        recs.insert(at + 1, (at, G_X_CONST | G_LIN, terms, 0, 0))
        cs.append(stream_case(d=16, tiles=3, kinds=1, recs=[r for k in range(16) for r in recs if r[0] == k]))
    cs.append(stream_case(d=8, tiles=3, recs=[(k, G_M_CONST | (G_LIN if k == 5 else 0), 4, k, 0) for k in range(8)]))   # rk from the gradient stream alone
    for kinds in (0, 1, 2, 3):
        for mode in (SPARSE, ANALYTIC, DENSE):
            cs.append(stream_case(d=8, tiles=3, mode=mode, kinds=kinds, recs=chain(8)))
            cs.append(stream_case(d=8, tiles=3, mode=mode, kinds=kinds, has_ss=0, recs=chain(8, flags=G_GEN)))
    cs.append(stream_case(tw=32)); cs.append(stream_case(gt=1)); cs.append(stream_case(recs=[])); cs.append(stream_case(mode=DENSE, has_ss=0)); cs.append(stream_case(mode=DENSE, kinds=2))
    cs.append(dict(kind="first", line="first"))
    return list({c["line"]: c for c in cs}.values())        # (the loops above meet a few configurations twice)


SAY1 = "fugue_amd: compiled HMC unit: d %d, task cost %d, resident %d, W %d\n"
SAY2 = "fugue_amd: compiled HMC unit: W %d, longest wave %d (tasks) / %d (whole coordinates), tiles per CU %d / %d\n"
TAILS = ("off", "off_an", "off_used", "c", "g")    # 17 entries that end in repeats of one value


def pack(out, names):
    """The fixture's form of a driver line: names by index, FG_JIT_VERBOSE's text as its numbers, the repeats at the end of off[] / c[] / g[] dropped."""
    o = {k: v for k, v in out.items() if k != "kind"}
    for k in ("name", "name2"):
        if k in o:
            if o[k] not in names:
                names.append(o[k])
            o[k] = names.index(o[k])
    if "say" in o:
        o["say"] = [int(x) for x in re.findall(r"-?\d+", o["say"])]               # (nine numbers with the first line, five without)
    for k in TAILS:
        if k in o:
            assert len(o[k]) == 17
            while len(o[k]) > 1 and o[k][-1] == o[k][-2]:
                o[k] = o[k][:-1]
    if "off_used" in o:
        o["off_used"] = "off_an" if o["off_used"] == o["off_an"] and o["off_used"] != o["off"] else ("off" if o["off_used"] == o["off"] else o["off_used"])
    if "gbins" in o:                                       # "=": the generated-behind part equals the prepared split's
        cur = {"gbins": cur_bins(o), "gcb": o["cb"], "gcbd": o["cb"]}
        for k in cur:
            if o[k] and o[k] == cur[k]:
                o[k] = "="
    return list(o.values()) if len(o) > 1 else next(iter(o.values()))


def cur_bins(o):
    """A split's 2 d tasks per wave, from order / off (off as packed or whole)."""
    off = o["off"] + [o["off"][-1]] * (17 - len(o["off"]))
    return [o["order"][off[w]:off[w + 1]] for w in range(o["W"])]


def unpack(kind, packed, names):
    keys = {"cost": ["cost"], "first": ["first"], "stream": ["rc", "W", "c", "g", "separable", "rk", "an", "ss", "name"],
            "mwi": ["rc", "W", "off", "order", "occ", "pl", "lds", "name", "occ2", "pl2", "lds2", "name2"],
            "jit": ["gbins", "gcb", "gcbd", "W", "off", "off_an", "off_used", "order", "cb", "say", "baked", "fused", "lds", "lds_eps", "name"]}[kind]
    o = dict(zip(keys, packed)) if isinstance(packed, list) and kind not in ("cost", "first") else {keys[0]: packed}
    for k in ("name", "name2"):
        if k in o:
            o[k] = names[o[k]]
    if isinstance(o.get("off_used"), str):
        o["off_used"] = o[o["off_used"]]
    for k in TAILS:
        if k in o:
            o[k] = o[k] + [o[k][-1]] * (17 - len(o[k]))
    if "gbins" in o:
        cur = {"gbins": cur_bins(o), "gcb": o["cb"], "gcbd": o["cb"]}
        for k in cur:
            if o[k] == "=":
                o[k] = cur[k]
    if "say" in o:
        v = o["say"]
        o["say"] = (SAY1 % tuple(v[:4]) + SAY2 % tuple(v[4:])) if len(v) == 9 else SAY2 % tuple(v)
    o["kind"] = kind
    return o


def cases_sha(cases):
    return hashlib.sha1("\n".join(c["line"] for c in cases).encode()).hexdigest()


def build_driver(out_dir, extra=()):
    exe = os.path.join(str(out_dir), "split_plan_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "split_plan_driver.cpp"), "-o", exe], check=True)
    return exe


def run_plans(exe, cases, work_dir):
    path = os.path.join(str(work_dir), "cases.txt")
    with open(path, "w") as f:
        f.write("".join(c["line"] + "\n" for c in cases))
    lines = subprocess.run([exe, path], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(cases)
    return [json.loads(ln) for ln in lines]


def ceil_div(a, b):
    return (a + b - 1) // b


def jit_rules(c, o):
    """The rules of fg_jit_task_plan / fg_jit_launch_shape this case reaches, from its inputs and the plan."""
    r = set()
    d, S, W = c["d"], c["S"], o["W"]
    waves, jocc, fused = c["sw"]
    forced = waves if waves != U else c["mw"]
    occ = jocc if jocc != U and 2 <= jocc <= 4 else 4
    wcap = min(16, 4 * occ, 2 * d)
    n_cu = max(1, c["n_simd"] // 4)
    if forced > 0:
        r.add("jit forced W")
        if forced > wcap:
            r.add("jit forced W clamped above")
    elif c["tiles"] <= n_cu:
        r.add("jit tiles <= n_cu")
    else:
        resident = [int(x) for x in re.findall(r"resident (\d+)", o["say"])][0]
        r.add("jit target 4" if resident >= 4 and 2 * d <= 16 else "jit target 8")
    if W == wcap and wcap < 2 * d:                         # (sixteen waves are four per SIMD: the cap of 16 and 4 occ at the default occupancy are one)
        r.add("jit wcap 16" if wcap == 16 else "jit wcap 4 occ")
    elif W == wcap and wcap < 4 * occ:
        r.add("jit wcap 2 d")
    spans = [int(x) for x in re.findall(r"-?\d+", o["say"].splitlines()[-1])][1:]     # span_tasks, span_coords, t1, t2
    lds2 = (2 * S + 3 * d + 2 + W) * 512
    room = spans[3] >= min(2, spans[2])
    if c["mode"] != DENSE:
        if fused == U:
            if o["cb"]:
                r.add("one barrier taken")
            elif room:
                assert spans[1] - spans[0] > 96
                r.add("one barrier refused: 96-unit span")
            else:
                r.add("one barrier refused: residency")
                if lds2 > LDS:
                    r.add("one barrier refused: lds2 > 160 KB")
        else:
            r.add("one barrier forced on" if fused != 0 and o["cb"] else "one barrier forced off" if fused == 0 else "one barrier forced on but lds2 > 160 KB")
    else:
        even = 2 * ceil_div(d, W) == ceil_div(2 * d, W)
        if o["cb"]:
            r.add("dense coordinate split taken")
        elif not even and (room if fused == U else fused != 0 and lds2 <= LDS):
            r.add("dense coordinate split refused: 2 ceil(d / W) != ceil(2 d / W)")
    if c["tasks"] == 0:
        assert o["gbins"] == [] and o["gcb"] == [] and o["gcbd"] == [] and o["baked"] == 0
        r.add("FG_JIT_TASKS=0")
    else:
        same = cur_bins(o) == o["gbins"]
        if c["mode"] == SPARSE:
            assert (o["baked"] != 0) == same and (o["baked"] == 2) == (bool(o["cb"]) and o["cb"] == o["gcb"]) and o["fused"] == (o["baked"] == 2)
            r.add("sparse: equal splits, baked %d" % o["baked"] if same else "sparse: unequal splits, baked 0")
        elif c["mode"] == DENSE:
            assert o["baked"] in (0, 3) and (o["baked"] == 3) == (bool(o["cb"]) and o["cb"] == o["gcbd"]) and o["fused"] == (o["baked"] == 3)
            r.add("dense: equal coordinate splits, baked 3" if o["baked"] else "dense: unequal or no coordinate splits, baked 0")
        else:
            assert o["baked"] == 0 and o["fused"] == 0
    assert ("one barrier per gradient" in o["name"]) == bool(o["fused"]) and ("(dense;" in o["name"]) == (c["mode"] == DENSE) and o["name"].startswith("k_hmc_jit_steps W=%d (" % W)
    assert o["lds"] == ((2 if o["fused"] else 1) * S + 3 * d + 2 + W) * 512 and o["lds_eps"] == (S + 3 * d + 2 + W) * 512
    if c["mode"] == ANALYTIC:
        assert o["off_used"] == (o["off_an"] if c["has_ad"] else o["off"])
        r.add("analytic: off_an" if c["has_ad"] else "analytic without the unit's derivative: off")
    else:
        assert o["off_used"] == o["off"]
    return r


def mwi_rules(c, o):
    r = set()
    if o["rc"] != 0:
        return {"interpreter: shrink loop reaches FG_E_UNSUPPORTED"}
    d, S, W = c["d"], c["S"], o["W"]
    priv = c["n_slots"] - S + 1
    rows = lambda w: (S + w * priv + 3 * d + 2 + w) * 512
    waves, occ_sw, _ = c["sw"]
    forced = waves if waves != U else c["mw"]
    occ = 4 if occ_sw == U else (2 if occ_sw <= 2 else 4)
    wcap = min(4 * occ, 2 * d)
    if forced > 0:
        r.add("interpreter forced W")
        if forced < 2:
            r.add("interpreter forced W clamped below")
        if forced > wcap:
            r.add("interpreter forced W clamped above")
        if W < max(2, min(forced, wcap)):
            r.add("interpreter: shrink loop lowers W")
    elif W < min(8, wcap) and 2 * W <= min(8, wcap):
        assert rows(2 * W) > LDS
        r.add("interpreter W doubling stopped by LDS")
    for q, (sw, tiles) in enumerate(((c["sw"], c["tiles"]), (c["sw2"], c["tiles2"]))):
        s = "2" if q else ""
        per_cu = ceil_div(tiles, max(1, c["n_simd"] // 4))
        total = rows(W) + c["prog_bytes"]
        assert o["occ" + s] == (4 if sw[1] == U else (2 if sw[1] <= 2 else 4))
        r.add("interpreter occ %d" % o["occ" + s])
        if sw[2] == U:
            r.add(("pl by the 80 KB rule: " if per_cu >= 2 else "pl by the 160 KB rule: ") + ("LDS" if o["pl" + s] else "global"))
        else:
            r.add("pl forced on" if o["pl" + s] else "pl forced off" if sw[2] == 0 else "pl forced on but beyond 160 KB")
        assert o["lds" + s] == (total if o["pl" + s] else rows(W))
        assert ("(program in global memory)" in o["name" + s]) == (not o["pl" + s]) and ("occ=2" in o["name" + s]) == (o["occ" + s] == 2) and o["name" + s].startswith("k_hmc_interp_mw_steps W=%d" % W)
    if c["sw2"] != c["sw"]:
        r.add("interpreter: a later launch keeps the split")
    return r


def stream_rules(c, o):
    r = set()
    if o["rc"] != 0:
        return {"stream: not this kernel's launch"}
    d, W = c["d"], o["W"]
    dense_stream = c["mode"] == DENSE
    if c["mw"] > 0:
        r.add("stream mw_override")
    else:
        resident = max(1, min(LDS // c["lds_bytes"], ceil_div(c["tiles"], max(1, c["n_simd"] // 4))))
        if W < 16 and resident * W < 16:
            assert d < 4 * W
            r.add("stream: resident W < 16 loop stopped by d >= 4 W")
        else:
            r.add("stream: resident W >= 16 or sixteen waves")
    if dense_stream and W > 1:
        assert o["c"][:W] == [d * w // W for w in range(W)] and o["g"][:W] == [0] * W
        r.add("stream: dense-stream cuts")
    if not dense_stream and W > 1:
        has_lin = any(rec[1] & G_LIN for rec in c["recs"])
        foreign = any((not rec[1] & G_X_CONST and not o["c"][w] <= rec[3] < o["c"][w + 1]) or (not rec[1] & G_M_CONST and not o["c"][w] <= rec[4] < o["c"][w + 1])
                      for w in range(W) for rec in c["recs"][o["g"][w]:o["g"][w + 1]])
        assert o["separable"] == (0 if has_lin or foreign else 1)
        r.add("stream: separable" if o["separable"] else "stream: separable 0 from a foreign operand" if foreign else "stream: separable 0 from a linear predictor")
    r.add("stream rk %d" % o["rk"])
    rk = max([c["kinds"]] + [2 if rec[1] & G_GEN else 1 if rec[1] & G_LIN else 0 for rec in c["recs"]]) if c["kinds"] < 2 else c["kinds"]
    if c["mode"] == ANALYTIC and rk == 2:
        assert o["rk"] == 0
        r.add("stream: analytic rk 2 -> 0")
    assert o["name"] == ("k_hmc_stream_steps (dense stream) W=%d" if dense_stream else "k_hmc_stream_steps W=%d") % W
    return r


RULES = {
    "jit forced W", "jit forced W clamped above", "jit tiles <= n_cu", "jit target 4", "jit target 8", "jit wcap 16", "jit wcap 4 occ", "jit wcap 2 d",
    "one barrier taken", "one barrier refused: 96-unit span", "one barrier refused: residency", "one barrier refused: lds2 > 160 KB", "one barrier forced on", "one barrier forced off",
    "one barrier forced on but lds2 > 160 KB", "dense coordinate split taken", "dense coordinate split refused: 2 ceil(d / W) != ceil(2 d / W)", "FG_JIT_TASKS=0",
    "sparse: equal splits, baked 1", "sparse: equal splits, baked 2", "sparse: unequal splits, baked 0", "dense: equal coordinate splits, baked 3", "dense: unequal or no coordinate splits, baked 0",
    "analytic: off_an", "analytic without the unit's derivative: off",
    "interpreter forced W", "interpreter forced W clamped below", "interpreter forced W clamped above", "interpreter: shrink loop lowers W", "interpreter W doubling stopped by LDS",
    "interpreter: shrink loop reaches FG_E_UNSUPPORTED", "interpreter occ 2", "interpreter occ 4", "pl by the 80 KB rule: LDS", "pl by the 80 KB rule: global", "pl by the 160 KB rule: LDS",
    "pl by the 160 KB rule: global", "pl forced on", "pl forced off", "pl forced on but beyond 160 KB", "interpreter: a later launch keeps the split",
    "stream: not this kernel's launch", "stream mw_override", "stream: resident W < 16 loop stopped by d >= 4 W", "stream: resident W >= 16 or sixteen waves", "stream: dense-stream cuts",
    "stream: separable", "stream: separable 0 from a foreign operand", "stream: separable 0 from a linear predictor", "stream rk 0", "stream rk 1", "stream rk 2", "stream rk 3",
    "stream: analytic rk 2 -> 0", "stream: a linear predictor's cost moves a cut",
}


def first_expected():
    """fg_hmc_jit_first over mode x jit_state x (gstream, gt, tw, sep gate, lin gate), in the driver's order -- the fixture holds the recorded table; this is its reading."""
    t = ""
    for mode in (DENSE, SPARSE, ANALYTIC):
        for js in (-1, 0, 1):
            for b in range(32):
                gstream, gt, tw32, sep, lin = (b & 1, b & 2, b & 4, b & 8, b & 16)
                t += "1" if mode == SPARSE and js >= 0 and (not gstream or not (gt or tw32 or sep or lin)) else "0"
    return t


def test_every_plan_is_the_recorded_one_and_every_rule_is_reached(tmp_path):
    assert shutil.which("g++"), "g++ builds the driver"
    fx = json.load(open(FIXTURE))
    cases = all_cases()
    assert os.path.getsize(FIXTURE) < 60 * 1024
    assert len(cases) == len(fx["cases"]) and cases_sha(cases) == fx["cases_sha1"], "the fixture was recorded for another list of cases"
    plans = run_plans(build_driver(tmp_path), cases, tmp_path)
    reached = {}
    for c, packed, got in zip(cases, fx["cases"], plans):
        assert got == unpack(c["kind"], packed, fx["names"]), c["line"]              # every field, the kernel's name byte for byte
        rules = {"jit": jit_rules, "mwi": mwi_rules, "stream": stream_rules}.get(c["kind"], lambda c, o: set())(c, got)
        for r in rules:
            reached[r] = reached.get(r, 0) + 1
    # a linear predictor of many terms moves its coordinate's cut against the same stream without it
    lin = [(c, o) for c, o in zip(cases, plans) if c["kind"] == "stream" and c["d"] == 16 and c["tiles"] == 3 and c["mw"] == 0]
    plain = [o for c, o in lin if not any(r[1] & G_LIN for r in c["recs"])]
    assert len(plain) == 1
    reached["stream: a linear predictor's cost moves a cut"] = sum(1 for c, o in lin if o["c"] != plain[0]["c"])
    assert set(reached) - RULES == set(), set(reached) - RULES
    assert {r: reached.get(r, 0) for r in RULES if not reached.get(r, 0)} == {}
    first = [o for c, o in zip(cases, plans) if c["kind"] == "first"]
    assert len(first) == 1 and len(first[0]["first"]) == 3 * 3 * 32 and first[0]["first"] == first_expected()


if __name__ == "__main__" and "--record" in sys.argv:
    import tempfile
    cases = all_cases()
    with tempfile.TemporaryDirectory() as td:
        exe = sys.argv[sys.argv.index("--record") + 1] if sys.argv[-1] != "--record" else build_driver(td)     # (another build of the driver's evaluation section)
        names = []
        packed = [pack(o, names) for c, o in zip(cases, run_plans(exe, cases, td))]
    fx = {"recorded_from": subprocess.run(["git", "-C", ROOT, "describe", "--always", "--dirty"], capture_output=True, text=True).stdout.strip(), "cases_sha1": cases_sha(cases), "names": names}
    if os.environ.get("FG_RECORDED_FROM"):
        fx["recorded_from"] = os.environ["FG_RECORDED_FROM"]
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(fx[k], separators=(",", ":")) for k in fx) +
                ',\n"cases": [\n' + ",\n".join(json.dumps(c, separators=(",", ":")) for c in packed) + "\n]}\n")
