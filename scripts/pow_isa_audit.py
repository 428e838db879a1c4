#!/usr/bin/env python3
"""Instruction audit of the PoW search loop (csrc/pow_search.hip, K1; reference hot loop miner.py:83-98).

Compiles the kernel TU for gfx950 to assembly (the build's flags, device side only), cuts out the loop body
of each ``pow_search_kernel`` instantiation (from the loop-header label to the hit branch) and classifies its
instructions: rotates (v_alignbit), 3-input logic (v_bitop3: XOR3 of the Sigma functions, Maj, Ch), 3-input
and 2-input adds, shifts (the schedule's >>3 / >>10), compares, and scalar instructions. Then compares the
count with a hand-derived floor of the same formulation (one nonce per lane, rounds 10..63 of the tail block,
schedule words W16..W63 with every nonce-independent term folded):

    per compression round   S1: 3 rotates + XOR3    S0: 3 rotates + XOR3    Ch + Maj: 2 bitop3
                            t1 = add3(h, S1, Ch) + add3(t1, K+W)   e = d + t1   a = add3(t1, S0, Maj)
    per schedule word        s0, s1: 2 rotates + shift + XOR3 each; W = add3 + add

For each loop it also prints how the two slow opcodes (v_alignbit_b32, v_add3_u32) are issued: a histogram of the
number of non-VALU instructions (s_sleep, s_nop, SALU) between a slow instruction and the VALU instruction before
it (0 / 1 / 2 or more: one is the cheapest, docs/PERF.md "PoW scalar slots"), and the s_mov_b32 and v_readlane_b32
counts of the audited path.

Usage: python scripts/pow_isa_audit.py [--out profiles/r6/pow_isa_r6.txt]
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = [('rotate (v_alignbit_b32)', r'^v_alignbit_b32'), ('bitop3 (XOR3 / Maj / Ch)', r'^v_bitop3_b32'),
           ('add3 (v_add3_u32)', r'^v_add3_u32'), ('add (v_add_u32)', r'^v_add_u32|^v_add_co_u32|^v_add_nc_u32'),
           ('shift (v_lshrrev_b32)', r'^v_lshrrev_b32|^v_lshlrev_b32'), ('bfi / cndmask', r'^v_bfi_b32|^v_cndmask'),
           ('compare', r'^v_cmp'), ('other VALU', r'^v_'), ('LDS', r'^ds_'), ('memory', r'^(global|buffer|flat)_'),
           ('filler (s_sleep / s_nop)', r'^s_sleep|^s_nop'), ('SALU / branch', r'^s_')]


def compile_asm() -> str:
    out = os.path.join(tempfile.mkdtemp(prefix='pow_isa_'), 'pow.s')
    subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', f'-I{ROOT}/csrc',
                    '--cuda-device-only', '-S', os.path.join(ROOT, 'csrc', 'pow_search.hip'), '-o', out], check=True,
                   stderr=subprocess.DEVNULL)
    return open(out).read()


HIT_TEST = r's_cbranch_exec(n)?z'
HIT_TEST_WAVE = r's_cbranch_vccn?z'  # variant 11: one branch per wave, taken when any lane has a hit
SLOW = r'^v_alignbit_b32|^v_add3_u32'


def fill_histogram(ins) -> dict:
    """{0, 1, 2: slow instructions with that many (2: two or more) non-VALU instructions directly in front}."""
    hist, gap = {0: 0, 1: 0, 2: 0}, 0
    for i in ins:
        if i.startswith('v_'):
            if re.match(SLOW, i):
                hist[min(gap, 2)] += 1
            gap = 0
        else:
            gap += 1
    return hist


def cheapest_path(loop: str, hit_test: str = HIT_TEST) -> list:
    """The instructions of one iteration that takes no optional work: the loop cut into basic blocks, and from
    the header to the block that ends in the hit test the path with the fewest VALU instructions. A loop of one
    block is that block. The split kernel (variant 10) recomputes lane constants in blocks of their own when a
    carry flips; the path found here is the iteration in which none does."""
    blocks, names = [[]], {}
    for ln in loop.splitlines():
        m = re.match(r'^(\.LBB\w+):', ln)
        if m:
            if blocks[-1]:
                blocks.append([])
            names[m.group(1)] = len(blocks) - 1
            continue
        if not re.match(r'^\s+[a-z]', ln) or ln.strip().startswith(';'):
            continue
        blocks[-1].append(ln.split())
        if re.match(r's_cbranch|s_branch', ln.split()[0]):
            blocks.append([])
    last = max((i for i, b in enumerate(blocks) if b and re.match(hit_test, b[-1][0])), default=len(blocks) - 1)
    cost = lambda b: (sum(1 for t in b if t[0].startswith('v_')), len(b))
    best = {0: (cost(blocks[0]), [0])}
    todo = [0]
    while todo:
        i = todo.pop()
        if i == last or not blocks[i]:
            succ = [] if i == last else [i + 1]
        else:
            op = blocks[i][-1]
            tgt = names.get(op[1]) if len(op) > 1 else None
            succ = [tgt] if op[0] == 's_branch' else [tgt, i + 1] if op[0].startswith('s_cbranch') else [i + 1]
        for j in succ:
            if j is None or j > last or j <= 0:
                continue
            c = tuple(a + b for a, b in zip(best[i][0], cost(blocks[j])))
            if j not in best or c < best[j][0]:
                best[j] = (c, best[i][1] + [j])
                todo.append(j)
    path = best.get(last, (None, list(range(last + 1))))[1]
    ins = [t[0] for i in path for t in blocks[i]]
    return ins[:-1] if ins and re.match(hit_test, ins[-1]) else ins


def loop_bodies(asm: str) -> dict:
    """{kernel symbol: (loop-body instruction mnemonics, NumVgprs, Occupancy)} for every search kernel."""
    out = {}
    for m in re.finditer(r'^(_ZN4upow\w*pow_search\w*):', asm, re.M):
        name = m.group(1)
        end = asm.find('.Lfunc_end', m.end())
        body = asm[m.end():end]
        tail = asm[end:asm.find('.end_amdhsa_kernel', end) if '.end_amdhsa_kernel' in asm[end:] else end + 4000]
        stats = asm[end:end + 6000]
        vg = re.search(r'; NumVgprs: (\d+)', stats)
        occ = re.search(r'; Occupancy: (\d+)', stats)
        # variant 12's loop lies in the claiming loop: its header line names the parent first
        hdr = re.search(r'^(\.LBB\w+):\s*;(?:\s*Parent Loop[^\n]*\n\s*;)? =>\s*This Inner Loop Header', body, re.M)
        if not hdr:
            continue
        loop = body[hdr.end():]
        stop = re.search(HIT_TEST, loop)  # the hit test: everything before it runs once per nonce
        back = re.search(r's_cbranch_\w+\s+' + re.escape(hdr.group(1)) + r'\b', loop)
        wave = [m for m in re.finditer(HIT_TEST_WAVE, loop[:back.start()] if back else '')]
        if wave and not (stop and back and stop.start() < back.start()):
            stop = wave[-1]  # the hit test is the last branch on vcc before the back edge
        loop = loop[:stop.end()] if stop else loop
        ins = cheapest_path(loop, stop.group(0) if stop else HIT_TEST)
        out[name] = (ins, int(vg.group(1)) if vg else None, int(occ.group(1)) if occ else None)
        del tail
    return out


def classify(ins):
    c = collections.OrderedDict((k, 0) for k, _ in CLASSES)
    for i in ins:
        for k, pat in CLASSES:
            if re.match(pat, i):
                c[k] += 1
                break
    return c


def floor_v2() -> dict:
    """The hand-derived VALU floor of the v2 search (see the module docstring)."""
    rounds = (63 - 11 + 1) * 14 - 1 + 2  # rounds 11..63 at 14 ops (e of round 63 unused), round 10: two adds
    # schedule: W16, W18, W20, W22 fold to constants; W17 and W24 are const + one nonce-dependent term
    sched = {17: 1, 19: 5, 21: 5, 23: 5, 24: 1, 25: 10, 26: 6, 27: 5, 28: 5, 29: 5, 30: 5, 31: 5}
    sched.update({i: 10 for i in range(32, 64)})
    return {'rounds': rounds, 'schedule': sum(sched.values()), 'total': rounds + sum(sched.values())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--asm', default=None, help='read this assembly file instead of compiling the kernel TU')
    a = ap.parse_args()
    asm = open(a.asm).read() if a.asm else compile_asm()
    lines = ['# PoW search loop: instructions per nonce (one loop iteration = one nonce per lane)',
             f'# source csrc/pow_search.hip, hipcc --offload-arch=gfx950 -O3 (scripts/pow_isa_audit.py)', '']
    for name, (ins, vgpr, occ) in loop_bodies(asm).items():
        c = classify(ins)
        valu = sum(v for k, v in c.items() if k not in ('LDS', 'memory', 'filler (s_sleep / s_nop)', 'SALU / branch'))
        lines.append(f'{name}  (VGPRs {vgpr}, occupancy {occ} waves/SIMD)')
        for k, v in c.items():
            if v:
                lines.append(f'    {k:28s} {v:5d}')
        lines.append(f'    {"VALU per nonce":28s} {valu:5d}')
        if any(i.startswith(('s_sleep', 's_nop')) for i in ins):
            h = fill_histogram(ins)
            lines.append(f'    slow opcodes by non-VALU instructions in front   0: {h[0]}   1: {h[1]}   2+: {h[2]}')
            lines.append(f'    s_mov_b32 {sum(i == "s_mov_b32" for i in ins)}   '
                         f'v_readlane_b32 {sum(i == "v_readlane_b32" for i in ins)}   '
                         f's_nop {sum(i == "s_nop" for i in ins)}')
        lines.append('')
    f = floor_v2()
    lines.append(f'hand-derived floor of the v2 formulation: {f["total"]} VALU per nonce '
                 f'({f["rounds"]} round ops + {f["schedule"]} schedule ops)')
    text = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text)
    sys.stdout.write(text)


if __name__ == '__main__':
    main()
