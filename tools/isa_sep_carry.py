"""Static look at k_hmc_sep_steps with the carried start gradient: a sibling of tools/isa_sep_scalar_state.py (which gives the transition
loop's mix of one instantiation) for what the carry's acceptance rule needs of EVERY instantiation, in two hipcc -S files of one source
line (parent, this commit):
  * the kernels' metadata side by side -- VGPRs, spilled VGPRs, scratch bytes per lane, SGPRs, spilled SGPRs -- and whether the two
    instruction streams are the same, instruction for instruction (labels, comments and directives left out);
  * per kernel, its leapfrog loops: innermost loops (no other backward branch inside) without LDS, memory or call instructions and
    with >= 8 v_add_f64 / v_mul_f64.
    For each: f64 instructions, other VALU instructions, scratch accesses, lane moves.
usage: python tools/isa_sep_carry.py parent.s new.s [name-substring-for-loop-detail]"""
import re, sys
from collections import Counter


def kernels(path):
    s = open(path).read()
    meta = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', s, re.S):
        g = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, m.group(2)).group(1))
        meta[m.group(1)] = (g('vgpr_count'), g('vgpr_spill_count'), g('private_segment_fixed_size'), g('sgpr_count'), g('sgpr_spill_count'))
    out = {}
    for f in re.split(r'\n(?=\S+:\s+; @)', s):
        m = re.match(r'(\S+):\s+; @', f)
        if not m or 'k_hmc_sep_steps' not in m.group(1) or m.group(1) not in meta: continue
        body = f.split('\n.Lfunc_end')[0]
        lines = [l for l in body.split('\n')]
        out[m.group(1)] = (meta[m.group(1)], lines)
    return out


def short(name):
    t = re.search(r'ILb(\d)ELi(\d)ELi(\d)ELi(\d)ELi(\d)ELb(\d)ELb(\d)ELb(\d)E', name)
    if not t: return name[:40]
    b = lambda x: 'true' if x == '1' else 'false'
    g = t.groups()
    return f"<{b(g[0])}, {g[1]}, {g[2]}, {g[3]}, {g[4]}, {b(g[5])}, {b(g[6])}{', ranged' if g[7] == '1' else ''}>"


def stream(lines):
    """the instructions alone, with branch targets as they are (a label renumbered by a new block elsewhere would show: it does not here)"""
    return [' '.join(l.split(';')[0].split()) for l in lines if l.startswith('\t') and not l.strip().startswith((';', '.'))]


def leapfrog_loops(lines):
    labels = {mm.group(1): i for i, l in enumerate(lines) if (mm := re.match(r'^(\.LBB\d+_\d+):', l))}
    res = []
    for i, l in enumerate(lines):
        mm = re.search(r's_c?branch\w*\s+(\.LBB\d+_\d+)', l)
        if not (mm and mm.group(1) in labels and labels[mm.group(1)] < i): continue
        body = lines[labels[mm.group(1)]:i + 1]
        ins = [b.split()[0] for b in body if b.startswith('\t') and not b.strip().startswith((';', '.'))]
        if any(o.startswith(('ds_', 'global_', 'flat_', 's_load', 's_swappc', 's_barrier')) for o in ins): continue
        lo = labels[mm.group(1)]
        inner = [re.search(r's_c?branch\w*\s+(\.LBB\d+_\d+)', b) for b in body[:-1]]
        if any(t and lo <= labels.get(t.group(1), -1) <= lo + k for k, t in enumerate(inner)): continue      # holds a loop of its own
        c = Counter(ins)
        if c['v_add_f64'] + c['v_mul_f64'] < 8: continue
        f64 = sum(v for k, v in c.items() if '_f64' in k)
        lanes = c['v_readlane_b32'] + c['v_writelane_b32']
        valu = sum(v for k, v in c.items() if k.startswith('v_'))
        res.append((f64, valu - f64 - lanes, sum(v for k, v in c.items() if k.startswith(('scratch_', 'buffer_'))), lanes,
                    bool(c['v_div_fmas_f64'] or c['v_cmp_class_f64'] or c['v_cmp_nlg_f64'] or c['v_rcp_f64'])))
    return res


A, B = kernels(sys.argv[1]), kernels(sys.argv[2])
detail = sys.argv[3] if len(sys.argv) > 3 else None
print("instantiation <MASS, MODE, HALF, NC, NOBS_R, U0_R, FOLD>   parent              | this commit          stream   leapfrog loops of this commit: f64+other VALU (c: checked), scratch accesses in them")
for name in sorted(A, key=short):
    if name not in B: continue
    (ma, la), (mb, lb) = A[name], B[name]
    same = stream(la) == stream(lb)
    loops = leapfrog_loops(lb)
    lp = ' '.join(f"{f}+{o}{'c' if chk else ''}" for f, o, s_, ln, chk in loops)
    scr = sum(s_ for f, o, s_, ln, chk in loops)
    print(f"{short(name):46s} {ma[0]:3d} {ma[1]:2d} {ma[2]:3d} {ma[3]:3d} {ma[4]:3d}   | {mb[0]:3d} {mb[1]:2d} {mb[2]:3d} {mb[3]:3d} {mb[4]:3d}   {'same  ' if same else 'DIFFER'}   {lp}  scratch-in-loops {scr}")
    if detail and detail in name:
        for tag, ls in (("parent", la), ("this commit", lb)):
            for f, o, s_, ln, chk in leapfrog_loops(ls):
                print(f"    {tag:12s} loop: f64 {f:3d}  other VALU {o:2d}  scratch {s_}  lane moves {ln}  {'(checked re-run)' if chk else ''}")
