"""The tiled decoder attention kernels (csrc/attn_tiled.hip) as the compiler leaves them: the resource summary of every
instantiation of the three kernel templates - head dim 32 / 64, causal / source mask, D / dQ pass - read back from the
assembly.  Numerics: test_attn_causal.py, test_attn_cross.py."""
import os
import re
import subprocess

import pytest

# DESIGN.md section 4 states these; a change of the kernels that moves them has to move the table too.
CAUSAL_OCCUPANCY = {('fwd', 64): 4, ('fwd', 32): 5, ('bwd_q', 64, 0): 4, ('bwd_q', 64, 1): 3, ('bwd_q', 32, 0): 5,
                    ('bwd_q', 32, 1): 4, ('bwd_kv', 64): 2, ('bwd_kv', 32): 4}
SOURCE_OCCUPANCY = {('fwd', 64): 4, ('fwd', 32): 5, ('bwd_q', 64, 0): 3, ('bwd_q', 64, 1): 2, ('bwd_q', 32, 0): 5,
                    ('bwd_q', 32, 1): 4, ('bwd_kv', 64): 2, ('bwd_kv', 32): 4}
OCCUPANCY = {(causal,) + key: occ for causal, table in ((1, CAUSAL_OCCUPANCY), (0, SOURCE_OCCUPANCY)) for key, occ in table.items()}


HIPCC = '/opt/rocm/bin/hipcc'


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_attn_tiled_kernels_use_no_scratch_and_keep_their_occupancy(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, 'm3p_amd', 'csrc', 'attn_tiled.hip')
    out = str(tmp_path / 'attn_tiled.s')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-munsafe-fp-atomics', '-ffp-contract=fast', '-S',
                    '--cuda-device-only', src, '-o', out], check=True, capture_output=True)
    text = open(out).read()
    seen = {}
    # template <int DH, bool CAUSAL> (and bool DQ on the query-block backward)
    for m in re.finditer(r'^(_Z\w*attn_(fwd|bwd_q|bwd_kv)_kernelILi(\d+)ELb([01])E(?:Lb([01])E)?\w*):.*?^; Kernel info:(.*?)^; COMPUTE_PGM_RSRC2',
                         text, re.S | re.M):
        kind, dh, causal, dq, info = m.group(2), int(m.group(3)), int(m.group(4)), m.group(5), m.group(6)
        key = (causal, kind, dh) if dq is None else (causal, kind, dh, int(dq))
        seen[key] = (int(re.search(r'ScratchSize: (\d+)', info).group(1)), int(re.search(r'Occupancy: (\d+)', info).group(1)))
    assert len(OCCUPANCY) == 16 and set(seen) == set(OCCUPANCY), sorted(seen)
    for key, (scratch, occ) in seen.items():
        assert scratch == 0, (key, scratch)
        assert occ == OCCUPANCY[key], (key, occ, OCCUPANCY[key])
