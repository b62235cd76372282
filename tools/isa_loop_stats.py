#!/usr/bin/env python3
"""Static instruction mix of the MFMA loops of a gfx950 .s file, per kernel: what one trip of the depth-tile loop
issues (MFMA / other vector / scalar / LDS / global), next to the whole kernel's static counts, registers, LDS and
scratch.  A loop is the set of blocks that the compiler's block comments assign to one loop header (blocks of loops nested in it,
the element-wise staging loops, are not counted); the loops that hold MFMAs are printed.  The depth-tile loop exists
twice per kernel: the shorter one is the loop with 16-byte loads only.
    hipcc --offload-arch=gfx950 -O3 -std=c++20 -Iinclude -Iuniver-ocr_amd/csrc <the file's hipcc-flags> \
          --cuda-device-only -S univer-ocr_amd/csrc/gemm_mfma.hip -o /tmp/gemm_mfma.s
    python tools/isa_loop_stats.py /tmp/gemm_mfma.s [name-filter]"""
import re
import sys
from collections import Counter

INSTR = re.compile(r'^\s+([a-z][a-z_0-9]+)\b')
BLOCK = re.compile(r'^(?:(\.LBB\d+_\d+):|; %bb\.\d+:)')
HEADER = re.compile(r'in Loop: Header=(BB\d+_\d+)')


def mix(lines):
    ops = Counter(m.group(1) for m in map(INSTR.match, lines) if m)
    out = Counter()
    for op, n in ops.items():
        if op.startswith('v_mfma'):
            out['mfma'] += n
        elif op.startswith('v_'):
            out['valu'] += n
            if op.startswith(('v_cndmask', 'v_cmp')):
                out['select'] += n
            if op.startswith('v_mov') or op.startswith('v_accvgpr'):
                out['mov'] += n
        elif op.startswith('ds_'):
            out['lds'] += n
            out['lds_write' if 'write' in op else 'lds_read'] += n
        elif op.startswith(('global_', 'flat_', 'buffer_', 'scratch_')):
            out['vmem'] += n
        elif op.startswith('s_'):
            out['salu'] += n
    return out


def fmt(c):
    return (f'mfma={c["mfma"]:4d} valu={c["valu"]:5d} (select={c["select"]:4d} mov={c["mov"]:4d}) salu={c["salu"]:5d} '
            f'lds={c["lds"]:4d} (r={c["lds_read"]:3d} w={c["lds_write"]:3d}) vmem={c["vmem"]:4d}')


def meta(key, text):
    m = re.search(r'[;.]\s*' + key + r':?\s+(\d+)', text)
    return m.group(1) if m else '?'


def short_name(name):
    s = re.sub(r'_ZN12_GLOBAL__N_1\d+', '', name)
    s = re.sub(r'EvT0_.*|Ev[A-Z].*', '', s)
    return re.sub(r'NS_(\d+)', '', s.replace('ILi', '<').replace('ELi', ','))


def main():
    text = open(sys.argv[1]).read()
    flt = sys.argv[2] if len(sys.argv) > 2 else ''
    for f in re.split(r'\n\s*\.globl\s+', text)[1:]:
        name = f.split('\n', 1)[0].split()[0]
        if flt not in name or 'cuid' in name or 'mfma' not in f:
            continue
        body = f.split('.section')[0].split('\n')
        # the compiler's own block comments say which loop a block belongs to (the innermost one)
        loops, current = {}, None
        for ln in body:
            m = BLOCK.match(ln)
            if m:
                label = m.group(1) or ''
                h = HEADER.search(ln)
                current = h.group(1) if h else (label.lstrip('.L') if 'Loop Header' in ln else None)
            if current:
                loops.setdefault(current, []).append(ln)
        print(f'{short_name(name)}\n    kernel        {fmt(mix(body))}  vgpr={meta("NumVgprs", f)} sgpr={meta("TotalNumSgprs", f)} '
              f'occupancy={meta("Occupancy", f)} scratch={meta("ScratchSize", f)} lds={meta("LDSByteSize", f)}')
        for header, lines in loops.items():
            c = mix(lines)
            if c['mfma']:
                print(f'    loop {header:8s} {fmt(c)}')


if __name__ == '__main__':
    main()
