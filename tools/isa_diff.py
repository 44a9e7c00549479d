#!/usr/bin/env python3
"""Kernel-by-kernel comparison of cross-compiled gfx950 assembly (no GPU):

    python tools/isa_diff.py OLD.s [OLD2.s ...] -- NEW.s [NEW2.s ...]

Each input (hipcc --cuda-device-only -S) is split into kernels by symbol; a kernel is its instruction stream (label to
.Lfunc_end) and its .amdhsa_kernel block.  What depends only on a function's position in its file is normalised away: the
function index in .LBB<i>_<j> / .LJTI<i>_<j> / .Lfunc_end<i>, __hip_cuid_*, comments and debug directives.  Prints the
number of kernels on each side, whether the two sets of names are the same, how many kernels are identical, and for every
other kernel the differing lines and its resource figures on both sides.  Exit status 0 only for the same set, all identical.
Used when code moves between files and must not change: profiles/gemm_split_isa.txt."""
import difflib, re, sys

LOCAL = re.compile(r'\.(LBB|LJTI|Lfunc_end|Lfunc_begin|Ltmp)(\d+)(_\d+)?')
DEBUG = ('.loc', '.file', '.cfi_', '.p2align', '.section', '.text', '.ident')
FIGURES = ('.amdhsa_next_free_vgpr', '.amdhsa_accum_offset', '.amdhsa_next_free_sgpr', '.amdhsa_private_segment_fixed_size',
           '.amdhsa_group_segment_fixed_size')


def norm(line):
    line = line.split(';', 1)[0].rstrip()
    line = LOCAL.sub(lambda m: '.' + m.group(1) + (m.group(3) or ''), line)
    return re.sub(r'__hip_cuid_\w+', '__hip_cuid', line)


def kernels(path):
    """name -> (instruction lines, .amdhsa_kernel lines, 'Occupancy' comment value)"""
    text = open(path).read().split('\n')
    names = [l.split()[1] for l in text if l.lstrip().startswith('.amdhsa_kernel ')]
    known = set(names)
    start = {l.split(':')[0]: i for i, l in enumerate(text) if l and not l[0].isspace() and l.split(':')[0] in known}
    out = {}
    for name in names:
        i = start[name] + 1
        body, desc, where = [], [], 0          # where: 0 instructions, 1 inside the .amdhsa_kernel block, 2 behind it
        while not text[i].startswith('.Lfunc_end'):
            l = norm(text[i]).strip()
            if l.startswith('.amdhsa_kernel '):
                where = 1
            if where == 1:
                desc.append(l)
            elif l and not l.startswith(DEBUG):
                body.append(l)
            if l.startswith('.end_amdhsa_kernel'):
                where = 2
            i += 1
        # (the '; Kernel info:' comment block follows .Lfunc_end, in front of the next function)
        occ = next((m.group(1) for m in (re.search(r'; Occupancy: (\d+)', text[j]) for j in range(i, min(i + 80, len(text)))) if m), None)
        assert occ is not None, '%s: no Occupancy figure behind %s' % (path, name)
        out[name] = (body, desc, occ)
    return out


def load(paths):
    all_k = {}
    for p in paths:
        for name, v in kernels(p).items():
            if name in all_k:
                sys.exit('%s: kernel %s occurs twice on one side' % (p, name))
            all_k[name] = v + (p,)
    return all_k


def figures(desc, occ):
    d = dict(l.split(None, 1) for l in desc if ' ' in l)
    return ', '.join('%s %s' % (f.replace('.amdhsa_', ''), d.get(f, '?')) for f in FIGURES) + ', occupancy ' + occ


def main():
    if '--' not in sys.argv:
        sys.exit(__doc__)
    cut = sys.argv.index('--')
    old, new = load(sys.argv[1:cut]), load(sys.argv[cut + 1:])
    print('kernels: %d old, %d new' % (len(old), len(new)))
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    print('same set of names: %s' % ('yes' if not only_old and not only_new else 'NO'))
    for n in only_old:
        print('  only old: %s' % n)
    for n in only_new:
        print('  only new: %s' % n)
    same, differ = [], []
    for n in sorted(set(old) & set(new)):
        (same if old[n][:2] == new[n][:2] else differ).append(n)
    print('identical instruction stream and kernel descriptor: %d of %d' % (len(same), len(same) + len(differ)))
    for n in same:
        print('  = %-110s %6d lines  %s' % (n, len(old[n][0]), new[n][3].rsplit('/', 1)[-1]))
    for n in differ:
        print('\n  DIFFERS %s (%s -> %s)' % (n, old[n][3], new[n][3]))
        print('    old: ' + figures(old[n][1], old[n][2]))
        print('    new: ' + figures(new[n][1], new[n][2]))
        d = list(difflib.unified_diff(old[n][0] + old[n][1], new[n][0] + new[n][1], 'old', 'new', lineterm='', n=1))
        for l in d[:80]:
            print('    ' + l)
        if len(d) > 80:
            print('    ... %d more diff lines' % (len(d) - 80))
    return 0 if not (only_old or only_new or differ) else 1


if __name__ == '__main__':
    sys.exit(main())
