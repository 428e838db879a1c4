#!/usr/bin/env python3
"""Dependency-distance audit of the PoW search loop (csrc/pow_search.hip), a sibling of pow_isa_audit.py.

Compiles the kernel TU for gfx950 to assembly, cuts out the loop body of one ``pow_search*`` kernel (loop
header to hit branch) and, from the mnemonics and registers of that body alone, reports for every VALU
instruction the distance, in issued VALU instructions, back to its nearest producer inside the iteration:

  * the histogram of distances, the count at distance 1 and 2;
  * the longest run of consecutive instructions that each depend on the one before;
  * for every schedule word W[i], how many rounds before round i it is produced.

How rounds and schedule words are recognised (no values are evaluated, only the data flow is followed):
  Sigma1 of a round is the XOR3 (v_bitop3 0x96) of three v_alignbit of one register by 6, 11 and 25; that
  register is the round's `e`, and the instruction that produced it closes the previous round. The loop has one
  such XOR3 per round and the last one belongs to round 63, which numbers them. A schedule word is a register
  read by a sigma0 (alignbit 7, 18, shift 3) or sigma1 (alignbit 17, 19, shift 10) group, or an add fed by such
  a group whose result goes into a round; its index is the round whose `e` first depends on it, minus one.

Usage: python scripts/pow_dep_audit.py [--kernel REGEX] [--out FILE]
"""
import argparse
import collections
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pow_isa_audit import compile_asm  # noqa: E402

DEFAULT_KERNEL = r'pow_search_pre_kernelILi2ELi8E'
SLOW = re.compile(r'^v_(alignbit_b32|add3_u32)')

Ins = collections.namedtuple('Ins', 'idx op dst src imm mod')


def regs(tok: str):
    """Register names of one operand: 'v[2:3]' -> v2, v3; 's7' -> s7; 'vcc' -> vcc; literals -> none."""
    tok = tok.strip()
    m = re.match(r'^([vs])\[(\d+):(\d+)\]$', tok)
    if m:
        return [f'{m.group(1)}{k}' for k in range(int(m.group(2)), int(m.group(3)) + 1)]
    if re.match(r'^[vs]\d+$', tok) or tok in ('vcc', 'exec'):
        return [tok]
    return []


def loop_valu(asm: str, kernel: str):
    """VALU instructions of the kernel's loop body in issue order, and the kernel's resource figures."""
    m = re.search(rf'^(_ZN4upow\w*{kernel}\w*):', asm, re.M)
    if not m:
        raise SystemExit(f'no kernel matching {kernel}')
    end = asm.find('.Lfunc_end', m.end())
    body, stats = asm[m.end():end], asm[end:end + 6000]
    hdr = re.search(r'^(\.LBB\w+):\s*; =>This Inner Loop Header', body, re.M)
    loop = body[body.index('\n', hdr.end()):]
    stop = re.search(r's_cbranch_execz', loop)
    loop = loop[:stop.start()] if stop else loop
    out, salu = [], 0
    for ln in loop.splitlines():
        ln = ln.split(';')[0].strip()
        if not ln or ln.endswith(':') or ln.startswith('.'):
            continue
        op, _, rest = ln.partition(' ')
        if not op.startswith('v_'):
            salu += 1
            continue
        toks = [t.strip().split(' ')[0] for t in rest.split(',')]
        ndst = 2 if '_co_' in op else 1
        dst = [r for t in toks[:ndst] for r in regs(t)]
        src = [r for t in toks[ndst:] for r in regs(t)]
        imm = [t for t in toks[ndst:] if not regs(t)]
        mod = rest.split(',')[-1].split()[1:]  # e.g. bitop3:0x96
        out.append(Ins(len(out), op, dst, src, imm, mod))
    res = {k: int(v) for k, v in re.findall(r'; (NumVgprs|TotalNumSgprs|ScratchSize|Occupancy): (\d+)', stats)}
    return m.group(1), out, salu, res


def distances(ins):
    """Per instruction: (distance to the nearest in-iteration VALU producer or None, producer indices)."""
    last, out = {}, []
    for i in ins:
        prod = sorted({last[r] for r in i.src if r in last})
        out.append((i.idx - prod[-1] if prod else None, prod))
        for r in i.dst:
            last[r] = i.idx
    return out


def rot_group(ins, deps, i, rots, shift):
    """If ins[i] is the XOR3 of rotates `rots` (and a right shift by `shift`, if not None) of ONE register,
    return (that register, index of its producer or None)."""
    if not ins[i].op.startswith('v_bitop3') or 'bitop3:0x96' not in ins[i].mod:
        return None
    want = set(rots) | ({('s', shift)} if shift is not None else set())
    got, base = set(), set()
    for p in deps[i][1]:
        q = ins[p]
        if q.op.startswith('v_alignbit') and len(set(q.src)) == 1 and q.imm:
            got.add(int(q.imm[-1], 0))
            base.add((q.src[0], tuple(deps[p][1])))
        elif q.op.startswith('v_lshrrev') and q.imm and q.src:
            got.add(('s', int(q.imm[0], 0)))
            base.add((q.src[-1], tuple(deps[p][1])))
    if got != want or len(base) != 1:
        return None
    reg, prod = next(iter(base))
    return reg, (prod[-1] if prod else None)


def schedule_lead(ins, deps):
    """[(word index, produced in round, lead in rounds)] for the schedule words found in the loop."""
    users = collections.defaultdict(list)
    for i in ins:
        for p in deps[i.idx][1]:
            users[p].append(i.idx)
    big1, small = [], {}  # Sigma1 markers: (xor3 idx, producer of e); sigma groups: xor3 idx -> producer of the word
    for i in ins:
        g = rot_group(ins, deps, i.idx, (6, 11, 25), None)
        if g:
            big1.append((i.idx, g[1]))
            continue
        for rots, sh in (((7, 18), 3), ((17, 19), 10)):
            g = rot_group(ins, deps, i.idx, rots, sh)
            if g:
                small[i.idx] = g[1]
    if not big1:
        return [], 0
    first_round = 64 - len(big1)
    # round r runs from after the producer of its `e` to the producer of round r+1's `e`
    closes = [p if p is not None else -1 for _, p in big1]  # closes[k]: last instruction of round first_round+k-1
    marker_round = {x: first_round + k for k, (x, _) in enumerate(big1)}

    def round_of(pos):
        r = first_round - 1
        for k, c in enumerate(closes):
            if pos > c:
                r = first_round + k
        return r

    def first_marker_below(start):
        """Smallest round whose Sigma1 depends on instruction `start`, not passing through sigma groups."""
        seen, todo, best = set(), [start], None
        while todo:
            n = todo.pop()
            for u in users[n]:
                if u in seen:
                    continue
                seen.add(u)
                if u in marker_round:
                    best = marker_round[u] if best is None else min(best, marker_round[u])
                    continue
                todo.append(u)
        return best

    sig_members = set()
    for x in small:
        sig_members.add(x)
        sig_members.update(deps[x][1])
    words = set(p for p in small.values() if p is not None)
    # words nothing takes a sigma of (the last ones): adds fed by a sigma group that are not fed into another
    # schedule add only
    for i in ins:
        if i.op.startswith('v_add') and any(p in small for p in deps[i.idx][1]):
            us = users[i.idx]
            if us and not all(ins[u].op.startswith('v_add') and any(p in small for p in deps[u][1]) for u in us):
                words.add(i.idx)
    out = []
    for w in sorted(words):
        # the round that consumes W[i] is i: its t1 feeds e of round i+1; follow only the non-sigma users
        best = None
        for u in users[w]:
            if u in sig_members:
                continue
            m = marker_round.get(u) or first_marker_below(u)
            if u in marker_round:
                m = marker_round[u]
            if m is not None:
                best = m if best is None else min(best, m)
        idx = (best - 1) if best is not None else 63
        out.append((idx, round_of(w), idx - round_of(w)))
    return sorted(out), first_round


def report(asm: str, kernel: str) -> str:
    name, ins, salu, res = loop_valu(asm, kernel)
    deps = distances(ins)
    hist = collections.Counter(d for d, _ in deps)
    run = best = 0
    best_at = 0
    for i, (d, _) in enumerate(deps):
        run = run + 1 if d == 1 else 0
        if run > best:
            best, best_at = run, i
    slow = sum(1 for i in ins if SLOW.match(i.op))
    L = [f'# dependency distances in the PoW loop body of {name}',
         '# hipcc --offload-arch=gfx950 -O3 (scripts/pow_dep_audit.py); distance = issued VALU instructions back to',
         '# the nearest producer of a source register within the iteration', '',
         f'VGPRs {res.get("NumVgprs")}  SGPRs {res.get("TotalNumSgprs")}  scratch {res.get("ScratchSize")}  '
         f'occupancy {res.get("Occupancy")} waves/SIMD',
         f'loop VALU {len(ins)} ({slow} SLOW alignbit/add3 + {len(ins) - slow} FAST), scalar in loop {salu}', '',
         'distance  instructions']
    for d in sorted(k for k in hist if k is not None):
        if d <= 16:
            L.append(f'{d:8d}  {hist[d]:5d}')
    L.append(f'{"17+":>8s}  {sum(v for k, v in hist.items() if k is not None and k > 16):5d}')
    L.append(f'{"none":>8s}  {hist.get(None, 0):5d}   (sources are SGPRs, constants or loop-carried)')
    known = [d for d, _ in deps if d is not None]
    L += ['', f'at distance 1: {hist.get(1, 0)}   at distance 2: {hist.get(2, 0)}   '
              f'at distance <= 2: {100.0 * (hist.get(1, 0) + hist.get(2, 0)) / len(ins):.1f} % of the loop',
          f'mean distance {sum(known) / len(known):.2f}, median {sorted(known)[len(known) // 2]}',
          f'longest run of consecutively dependent instructions: {best + 1 if best else 0} '
          f'(ending at loop VALU #{best_at})']
    # distance-1 pairs by opcode class of producer -> consumer
    pairs = collections.Counter()
    for i, (d, _) in enumerate(deps):
        if d == 1:
            pairs[('SLOW' if SLOW.match(ins[i - 1].op) else 'FAST') + ' -> ' +
                  ('SLOW' if SLOW.match(ins[i].op) else 'FAST')] += 1
    L.append('distance-1 pairs by class: ' + ', '.join(f'{k} {v}' for k, v in sorted(pairs.items())))
    lead, first_round = schedule_lead(ins, deps)
    L += ['', f'schedule words: rounds between production and the consuming round (first round in the loop: '
              f'{first_round})', 'word  produced in round  lead']
    for idx, r, ld in lead:
        L.append(f'W{idx:<4d} {r:17d}  {ld:4d}')
    if lead:
        lds = [ld for _, _, ld in lead]
        L.append(f'words {len(lead)}, mean lead {sum(lds) / len(lds):.2f} rounds, min {min(lds)}, max {max(lds)}')
    return '\n'.join(L) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernel', default=DEFAULT_KERNEL, help='regex inside the mangled kernel name')
    ap.add_argument('--asm', default=None, help='read this assembly file and do not compile')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    asm = open(a.asm).read() if a.asm else compile_asm()
    text = report(asm, a.kernel)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text)
    sys.stdout.write(text)


if __name__ == '__main__':
    main()
