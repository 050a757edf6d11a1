"""Resource guard of the bed DRC kernel (csrc/mk_cascade_adjoint.h:
k_bed_adjoint), read from the built library's gfx950 code object with the ROCm
LLVM tools (no GPU), as tests/test_cascade_kernel_budget.py does it; and its
LDS formula, read from the header."""
import os
import re

import pytest

from pycatkin_amd import _lib
from test_cascade_kernel_budget import LLVM, _kernel_metadata

CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'csrc')


@pytest.mark.skipif(not (os.path.isfile(_lib.LIB_PATH) and os.path.isfile(LLVM + '/llvm-readelf')),
                    reason='library or ROCm LLVM tools absent')
def test_bed_adjoint_register_budget(tmp_path):
    """One instance, no scratch (private_segment_fixed_size 0), and at most 168
    VGPRs + AGPRs: 3 waves per SIMD, what 3 blocks per CU at NS 6 need (the
    shipped figure, DESIGN.md "Bed DRC": 153 VGPRs, 0 AGPRs, 0 B); its sibling
    k_lane_multi_adjoint keeps its own zero."""
    md = _kernel_metadata(_lib.LIB_PATH, tmp_path)
    bed = {k: v for k, v in md.items() if 'k_bed_adjoint' in k}
    assert len(bed) == 1, sorted(bed)
    (vg, ag, priv), = bed.values()
    assert priv == 0, priv
    assert vg + ag <= 168, (vg, ag)
    sib = [v for k, v in md.items() if 'k_lane_multi_adjoint' in k]
    assert len(sib) == 1 and sib[0][2] == 0


def test_lds_formula():
    """LDS per block is 16 (NS^2 + 2 NS) 64 bytes, the one-lane multi kernel's,
    sized by NS alone: the header's formula, and what the launch passes."""
    txt = open(os.path.join(CSRC, 'mk_cascade_adjoint.h')).read()
    m = re.search(r'cascade_adjoint_lds_bytes\(int NS\)\s*\{\s*return\s*([^;]+);', txt)
    assert m and re.sub(r'\s+', '', m.group(1)) == '(size_t)(NS*NS+2*NS)*64*sizeof(dd)'
    sib = open(os.path.join(CSRC, 'mk_sens_multi_lane.h')).read()
    assert 'multi_lane_entries(int NS) { return NS * NS + 2 * NS; }' in sib
    host = open(os.path.join(CSRC, 'mk_kernels.hip')).read()
    assert 'launch_adjoint(k_bed_adjoint, 64, cascade_adjoint_lds_bytes(NS)' in host
    # 160 KiB of LDS per CU: 6 / 3 / 2 blocks at NS 4 / 6 / 8
    assert [160 * 1024 // (16 * (ns * ns + 2 * ns) * 64) for ns in (4, 6, 8)] == [6, 3, 2]
    # no barrier, no atomics in the kernel
    body = txt[txt.index('__launch_bounds__(64) k_bed_adjoint'):]
    assert '__syncthreads' not in body and 'wsync' not in body and 'atomic' not in body
