"""Static look at the scalar state of k_hmc_sep_steps in a hipcc -S file: per kernel, the registers and spills of its metadata, its
v_readlane / v_writelane (SGPRs parked in VGPR lanes) ahead of, inside and behind the transition loop, and the instruction mix of the
transition loop.  The loop is taken from the control-flow graph (every block that lies on a path from the loop's head back to it;
the largest such loop that holds a barrier), so where the compiler places a cold block does not move the counts.
Cold blocks -- the checked re-run, wave 0's accept step, the Welford push -- belong to the loop: the counts compare two builds of one
instantiation and are not the length of a path.  "hot" leaves out the blocks of the checked re-run (those with a v_rcp_f64 or v_div_*,
and the loops that hold v_cmp_nlg_f64 / v_cmp_class: the per-step "force is finite" test).
usage: python tools/isa_sep_scalar_state.py file.s [name-substring]"""
import re, sys
from collections import Counter
s = open(sys.argv[1]).read()
pat = sys.argv[2] if len(sys.argv) > 2 else "k_hmc_sep_steps"
meta = {}
for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', s, re.S):
    g = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, m.group(2)).group(1))
    meta[m.group(1)] = (g('sgpr_count'), g('sgpr_spill_count'), g('vgpr_count'), g('vgpr_spill_count'), g('private_segment_fixed_size'))
LANE = ('v_readlane_b32', 'v_writelane_b32')
lanes = lambda c: sum(c[k] for k in LANE)
cls = lambda c, p: sum(v for k, v in c.items() if k.startswith(p))
for f in re.split(r'\n(?=\S+:\s+; @)', s):
    m = re.match(r'(\S+):\s+; @', f)
    if not m or pat not in m.group(1): continue
    name = m.group(1)
    lines = f.split('\n')
    # basic blocks: a label starts one, a branch ends one
    blocks, cur = [], {'label': None, 'ops': [], 'succ': [], 'start': 0}
    for i, l in enumerate(lines):
        lm = re.match(r'^(\.LBB\d+_\d+):', l)
        if lm:
            if cur['ops'] or cur['label']: blocks.append(cur)
            cur = {'label': lm.group(1), 'ops': [], 'succ': [], 'start': i, 'ft': True}
            continue
        if not l.startswith('\t') or l.strip().startswith((';', '.')): continue
        o = l.split()[0]
        cur['ops'].append(o)
        bm = re.match(r'\s+s_(c?)branch\w*\s+(\.LBB\d+_\d+)', l)
        if bm or o in ('s_endpgm', 's_setpc_b64'):
            if bm: cur['succ'].append(bm.group(2))
            cur['ft'] = bool(bm and bm.group(1))
            blocks.append(cur)
            cur = {'label': None, 'ops': [], 'succ': [], 'start': i + 1, 'ft': True}
    blocks.append(cur)
    idx = {b['label']: k for k, b in enumerate(blocks) if b['label']}
    succ = [[idx[t] for t in b['succ'] if t in idx] + ([k + 1] if b.get('ft', True) and k + 1 < len(blocks) else []) for k, b in enumerate(blocks)]
    pred = [[] for _ in blocks]
    for k, ss in enumerate(succ):
        for t in ss: pred[t].append(k)
    # the transition loop: the largest natural loop (blocks that reach a backward branch to the head without passing the head) that holds
    # a barrier and not the kernel's entry (a cold block placed behind the kernel that jumps back up is no loop)
    def natural(head):
        body, work = {head}, [k for k in pred[head] if k >= head]
        while work:
            k = work.pop()
            if k in body: continue
            body.add(k)
            work.extend(pred[k])
        return body
    body = None
    for head in sorted({t for k, ss in enumerate(succ) for t in ss if t <= k}):
        b = natural(head)
        if 0 in b or not any('s_barrier' in blocks[q]['ops'] for q in b): continue
        if body is None or len(b) > len(body): body = b
    if body is None: continue
    reach, work = set(), [0]                                    # (blocks only reachable through the loop are behind it)
    while work:
        k = work.pop()
        if k in reach or k in body: continue
        reach.add(k); work.extend(succ[k])
    cold = {k for k in body if any(o.startswith(('v_rcp_f64', 'v_div_', 'v_cmp_nlg_f64', 'v_cmp_class_f64')) for o in blocks[k]['ops'])}
    cnt = lambda ks: Counter(o for k in ks for o in blocks[k]['ops'])
    pro, loop, hot = cnt(reach), cnt(body), cnt(body - cold)
    epi = cnt(set(range(len(blocks))) - reach - body)
    tmpl = re.search(r'ILb(\d)ELi(\d)ELi(\d)ELi(\d)ELi(\d)ELb(\d)ELb(\d)ELb(\d)E', name)
    short = "<" + ", ".join(tmpl.groups()) + ">" if tmpl else name[:40]
    sg, sgs, vg, vgs, scr = meta.get(name, (0, 0, 0, 0, 0))
    mix = lambda c: (f"VALU {cls(c, 'v_') - lanes(c):4d} (f64 {sum(v for k, v in c.items() if '_f64' in k):3d} cndmask {cls(c, 'v_cndmask'):2d} v_cmp {cls(c, 'v_cmp'):2d} mov {cls(c, 'v_mov_b32'):2d}) "
                     f"lanes {lanes(c):3d} SALU {cls(c, 's_') - cls(c, 's_load'):4d} s_load {cls(c, 's_load'):2d} LDS {cls(c, 'ds_'):3d}")
    print(f"{short:26s} sgpr {sg:3d} sgpr_spill {sgs:3d} vgpr {vg:3d} vgpr_spill {vgs:2d} scratch {scr:3d} | lanes: kernel {lanes(pro) + lanes(loop) + lanes(epi):3d} = ahead {lanes(pro):3d} "
          f"+ loop {lanes(loop):3d} + behind {lanes(epi):3d}\n    loop {mix(loop)} calls {loop['s_swappc_b64']}\n    hot  {mix(hot)}")
