#!/usr/bin/env python3
"""Generates the K-tile bodies of the two four-wave GEMM kernels (the unrolled MFMA / memory-instruction schedule): the
four files m3p_amd/csrc/gen/*.inc that gemm_nt_w4.hpp and gemm_wgrad_w4.hpp (parts of gemm.hip) include.  The schedule is
data here: which MFMA index is followed by which fragment read or LDS-DMA piece.  The kernels themselves are ordinary source
in those two files.
  gen_w4.py           writes the four files
  gen_w4.py --check   exits non-zero if a committed file is not what the generator makes (tests/test_kernel_isa.py)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

def mfma_lines(frag_a, frag_w, extra):
    out, n = [], 0
    for i in range(8):
        for j in range(8):
            l = '      W4_M(%s, %s, %d, %d);' % (frag_a, frag_w, i, j)
            if n in extra:
                l += ' ' + ' '.join(extra[n])
            out.append(l)
            n += 1
    return "\n".join(out)

def add(d, n, stmt):
    d.setdefault(n, []).append(stmt)

# ---- weight-gradient kernel: a "read" here is one fragment = two tr16 reads
def wg_mfma_lines(yf, xf, extra):
    out, n = [], 0
    for b in range(8):
        for a in range(8):
            l = '      WG_M(%s, %s, %d, %d);' % (yf, xf, b, a)
            if n in extra:
                l += ' ' + ' '.join(extra[n])
            out.append(l)
            n += 1
    return "\n".join(out)


# ---- the NT kernel's one-piece K-tile: slots are MFMA indices 0..127 (k-step 0 = 0..63)
KT_BAR1 = int(os.environ.get('W4_BAR1', '20'))          # after this MFMA: W of the stage is dead
KT_BAR2 = int(os.environ.get('W4_BAR2', '50'))          # ... and A
KT_BAR3 = int(os.environ.get('W4_BAR3', '107'))         # the next K-tile has landed
KT_DMA_W = [int(x) for x in os.environ.get('W4_DMA_W', '21,26,31,36,41,46,52,57').split(',')]
KT_DMA_A = [int(x) for x in os.environ.get('W4_DMA_A', '62,67,72,77,82,87,92,97').split(',')]
kt = {}
for r in range(8):                                      # W fragments of k-step 1: MFMAs 1..15
    add(kt, 2 * r + 1, 'M3P_DSR(fw1[%d], rb1, %d);' % (r, r * 2048))
a_slots = [17, 19] + [23 + 4 * k for k in range(6)]     # A fragments: two before the first barrier, the rest between the W transfers
for r, sl in enumerate(a_slots):
    add(kt, sl, 'M3P_DSR(fa1[%d], ra1, %d);' % (r, r * 2048))
n_after = sum(1 for sl in a_slots if sl <= KT_BAR1)
BAR_LAG = int(os.environ.get('W4_BAR_LAG', '0'))        # 1: one MFMA between a wait and its barrier (the pipe has work while the wave waits)
if BAR_LAG:
    add(kt, KT_BAR1, 'M3P_WAIT_LGKM(%d);' % n_after); add(kt, KT_BAR1 + 1, 'M3P_BAR();')
else:
    add(kt, KT_BAR1, 'M3P_WAIT_LGKM(%d); M3P_BAR();' % n_after)
for k, sl in enumerate(KT_DMA_W):
    add(kt, sl, 'W4_L(%d);' % (8 + k))
assert max(a_slots) < KT_BAR2
if BAR_LAG:
    add(kt, KT_BAR2, 'M3P_WAIT_LGKM(0);'); add(kt, KT_BAR2 + 1, 'M3P_BAR();')
else:
    add(kt, KT_BAR2, 'M3P_WAIT_LGKM(0); M3P_BAR();')
for k, sl in enumerate(KT_DMA_A):
    add(kt, sl, 'W4_L(%d);' % k)
add(kt, max(KT_DMA_A) + 1, 'W4_LD();')
assert max(KT_DMA_A) + 1 < KT_BAR3
if BAR_LAG:
    add(kt, KT_BAR3 - 1, 'M3P_WAIT_VM(16);'); add(kt, KT_BAR3, 'M3P_BAR();')
else:
    add(kt, KT_BAR3, 'M3P_WAIT_VM(16); M3P_BAR();')
for r in range(16):                                     # k-step 0 of the next K-tile
    add(kt, KT_BAR3 + 1 + r, ('M3P_DSR(fw0[%d], rb0n, %d);' % (r, r * 2048)) if r < 8 else ('M3P_DSR(fa0[%d], ra0n, %d);' % (r - 8, (r - 8) * 2048)))
assert KT_BAR3 + 16 <= 127
add(kt, 127, 'M3P_WAIT_LGKM(0);')
kt_a = {n: v for n, v in kt.items() if n < 64}
kt_b = {n - 64: v for n, v in kt.items() if n >= 64}

# ---- the weight-gradient kernel's one-piece K-tile: the NT kernel's slots, a "read" = one fragment
wkt = {}
for c in range(8):                                      # first operand's fragments of k-step 1
    add(wkt, 2 * c + 1, 'WG_YRD(%d, s_cur, 1);' % c)
for c, sl in enumerate(a_slots):                        # second operand's: two before the first barrier (= 4 read instructions)
    add(wkt, sl, 'WG_TR2(xl[%d], xh[%d], x_addr[s_cur][%d], 16384);' % (c, c, c))
add(wkt, KT_BAR1, 'M3P_WAIT_LGKM(%d); M3P_BAR();' % (2 * n_after))
for k, sl in enumerate(KT_DMA_W):
    add(wkt, sl, 'WG_L(%d);' % k)                       # (the first operand's region is pieces 0..7 here)
add(wkt, KT_BAR2, 'M3P_WAIT_LGKM(0); WG_SET1(); M3P_BAR();')
for k, sl in enumerate(KT_DMA_A):
    add(wkt, sl, 'WG_L(%d);' % (8 + k))
add(wkt, max(KT_DMA_A) + 1, 'WG_LD();')
WGK_BAR3 = int(os.environ.get('WGK_BAR3', str(KT_BAR3)))    # (a fragment is two read instructions here: the tail may want more room)
WGK_RSTEP = int(os.environ.get('WGK_RSTEP', '1'))
assert max(KT_DMA_A) + 1 < WGK_BAR3 and WGK_BAR3 + 1 + 15 * WGK_RSTEP <= 126
add(wkt, WGK_BAR3, 'M3P_WAIT_VM(16); M3P_BAR();')
for r in range(16):
    add(wkt, WGK_BAR3 + 1 + r * WGK_RSTEP, ('WG_YRD(%d, s_cur ^ 1, 0);' % r) if r < 8 else ('WG_TR2(xl[%d], xh[%d], x_addr[s_cur ^ 1][%d], 0);' % (r - 8, r - 8, r - 8)))
add(wkt, 127, 'M3P_WAIT_LGKM(0); WG_SET0();')
# Bias sums of the whole-tile launch (WG_BW / WG_BD expand to nothing unless the K-tile body is a BMODE 1 / 2 one).  The weights'
# reads go where an existing wait covers them, in order, at no other count: k-step 0's at MFMA 0, in front of every fragment
# read the lgkmcnt(4) of KT_BAR1 leaves behind; k-step 1's right after that barrier, in front of the reads lgkmcnt(0) of KT_BAR2
# waits for.  The 2 x 16 dot instructions - one per MFMA, between matrix instructions - take the slots that hold nothing else:
# k-step 0's from its weights' wait on, k-step 1's from KT_BAR2 on (its fragments are set there) and clear of the tail's
# fragment reads; consecutive ones go to different accumulators.
add(wkt, 0, 'WG_BW(0);')
add(wkt, KT_BAR1 + 1, 'WG_BW(1);')
for ks, start in ((0, KT_BAR1 + 2), (1, KT_BAR2 + 1)):
    dots = ['WG_BD(%d, %d, %d);' % (ks, j, dw) for dw in range(4) for j in range(4)]
    free = [n for n in range(start, WGK_BAR3) if n not in wkt]
    assert len(free) >= len(dots)
    for stmt, n in zip(dots, free):
        add(wkt, n, stmt)
wkt_a = {n: v for n, v in wkt.items() if n < 64}
wkt_b = {n - 64: v for n, v in wkt.items() if n >= 64}

OUT = os.path.join(ROOT, 'm3p_amd', 'csrc', 'gen')
files = {
    'nt_w4_ktile_a.inc': mfma_lines('fa0', 'fw0', kt_a),
    'nt_w4_ktile_b.inc': mfma_lines('fa1', 'fw1', kt_b),
    'wgrad_w4_ktile_a.inc': wg_mfma_lines('yf0', 'xf0', wkt_a),
    'wgrad_w4_ktile_b.inc': wg_mfma_lines('yf1', 'xf1', wkt_b),
}
stale = []
for name, body in files.items():
    text = '// generated, edit tools/gen/gen_w4.py\n' + body + '\n'
    p = os.path.join(OUT, name)
    if '--check' in sys.argv:
        if not os.path.exists(p) or open(p).read() != text:
            stale.append(name)
    else:
        os.makedirs(OUT, exist_ok=True)
        open(p, 'w').write(text)
if stale:
    sys.exit('m3p_amd/csrc/gen/{%s} out of date: run tools/gen/gen_w4.py' % ', '.join(stale))
if '--check' not in sys.argv:
    print('generated', ', '.join('%s (%d lines)' % (n, len(b.splitlines())) for n, b in files.items()))
