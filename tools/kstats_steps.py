#!/usr/bin/env python3
"""Per-kernel before/after table of two rocprofv3 --kernel-trace runs of bench.py, over the LAST N steps of each (the format of
profiles/*_kernel_stats.csv).  A step runs from one launch of the marker kernel (once per step) to the next.
    python tools/kstats_steps.py parent_kernel_trace.csv new_kernel_trace.csv [--steps 10] [--marker 'gemm_wgrad_w4_kernel<true>']"""
import csv
import re
import sys

args = [a for a in sys.argv[1:] if not a.startswith('--')]
steps = int(sys.argv[sys.argv.index('--steps') + 1]) if '--steps' in sys.argv else 10
marker = sys.argv[sys.argv.index('--marker') + 1] if '--marker' in sys.argv else 'gemm_wgrad_w4_kernel<true>'
if '--steps' in sys.argv:
    args.remove(str(steps))
if '--marker' in sys.argv:
    args.remove(marker)


def short(name):
    name = re.sub(r'\(anonymous namespace\)::|^void ', '', name)
    depth, out = 0, ''
    for ch in name:                 # cut the argument list, keep the template arguments
        if ch == '(' and depth == 0:
            break
        depth += ch == '<'
        depth -= ch == '>'
        out += ch
    return out.replace(', ', '; ')[:80]


def load(path):
    rows = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp']), short(r['Kernel_Name'])) for r in csv.DictReader(open(path)))
    marks = [i for i, r in enumerate(rows) if r[2] == marker]
    lo, hi = marks[-1 - steps], marks[-1]
    per = {}
    for s, e, n in rows[lo:hi]:
        per.setdefault(n, []).append((e - s) / 1e3)
    busy = sum(sum(v) for v in per.values()) / steps
    span = (rows[hi][0] - rows[lo][0]) / 1e3 / steps
    return per, busy, span


(a, abusy, aspan), (b, bbusy, bspan) = load(args[0]), load(args[1])
print('# kernel time per step: parent %.1f us, new %.1f us; marker to marker per step: parent %.1f, new %.1f' % (abusy, bbusy, aspan, bspan))
print('kernel,parent_per_step,parent_us_per_step,parent_avg_us,parent_min_us,parent_max_us,new_per_step,new_us_per_step,new_avg_us,'
      'new_min_us,new_max_us,delta_us_per_step')


def cols(v):
    if not v:
        return '0.0,0.0,,,'
    return '%.1f,%.1f,%.1f,%.1f,%.1f' % (len(v) / steps, sum(v) / steps, sum(v) / len(v), min(v), max(v))


for k in sorted(set(a) | set(b), key=lambda k: -max(sum(a.get(k, [])), sum(b.get(k, [])))):
    print('%s,%s,%s,%.1f' % (k, cols(a.get(k)), cols(b.get(k)), (sum(b.get(k, [])) - sum(a.get(k, []))) / steps))
