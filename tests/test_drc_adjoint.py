"""CPU-side checks of the analytic degree of rate control: the C-ABI's two
entry points (pck_drc_at, pck_drc_adjoint), the method switch of
System.drc_batch, the kernel's code-object metadata and the arbitrary-
precision restatement the GPU tests are measured against (tests/_sens.py)."""
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from oracle import mk_oracle as O
from pycatkin_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LLVM = '/opt/rocm/lib/llvm/bin'


def test_header_declares_the_entry_points():
    txt = open(os.path.join(ROOT, 'include', 'pycatkin_amd.h')).read()
    assert re.search(r'\bint pck_drc_at\(', txt) and re.search(r'\bint pck_drc_adjoint\(', txt)
    assert re.search(r'#define PCK_ST_SENS_SINGULAR 7\b', txt)
    assert '#define PCK_ABI_VERSION %d' % _lib.ABI_VERSION in txt and _lib.ABI_VERSION >= 9
    assert _lib.ST_SENS_SINGULAR == 7
    # each entry point cites the reference routine it replaces
    for name in ('pck_drc_at', 'pck_drc_adjoint'):
        doc = txt[:txt.index('int %s(' % name)]
        assert 'old_system.py:490' in doc[doc.rindex('/*'):]


def test_library_exports_the_entry_points():
    import ctypes
    import torch  # noqa: F401  (the library binds to torch's HIP runtime, pycatkin_amd/_lib.py)
    assert 'pck_drc_at' in _lib.EXPORTED and 'pck_drc_adjoint' in _lib.EXPORTED
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('pck_drc_at', 'pck_drc_adjoint'):
        getattr(lib, name)


def test_method_argument_is_checked(inputs):
    import pycatkin_amd as P
    s = P.read_from_input_file(os.path.join(inputs, 'DMTM', 'input.json'))
    with pytest.raises(ValueError):
        s.drc_batch(('r5', 'r9'), T=[500.0], steady=False, method='analytic')
    with pytest.raises(ValueError):
        s.drc_batch(('r5', 'r9'), T=[500.0], steady=True, method='x')
    with pytest.raises(ValueError):
        s.degree_of_rate_control(['r5', 'r9'], ss_solve=False, method='analytic')


def test_adjoint_kernels_use_no_scratch(tmp_path):
    """The matrix lives in LDS and no per-lane array has a run-time index:
    the code object's notes report private_segment_fixed_size == 0 for the
    three k_drc_adjoint<G> instances."""
    cp, fb, elf = str(tmp_path / 'lib_copy.so'), str(tmp_path / 'fb.bin'), str(tmp_path / 'k.elf')
    shutil.copyfile(_lib.LIB_PATH, cp)
    subprocess.run(['objcopy', '--dump-section', '.hip_fatbin=' + fb, cp], check=True)
    blob = open(fb, 'rb').read()
    starts = [m.start() for m in re.finditer(re.escape(b'__CLANG_OFFLOAD_BUNDLE__'), blob)]
    assert starts, 'no offload bundle in the library'
    found = {}
    for i, a in enumerate(starts):
        part = str(tmp_path / ('fb%d.bin' % i))
        open(part, 'wb').write(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        subprocess.run([LLVM + '/clang-offload-bundler', '--type=o', '--input=' + part,
                        '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--output=' + elf, '--unbundle'], check=True)
        notes = subprocess.run([LLVM + '/llvm-readelf', '--notes', elf], check=True, capture_output=True,
                               text=True).stdout
        for b in notes.split('  - .agpr_count:')[1:]:
            name = re.search(r'\.name:\s+(\S+)', b).group(1)
            if 'k_drc_adjoint' in name:
                found[name] = int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', b).group(1))
    assert len(found) == 3 and set(found.values()) == {0}, found


def test_restatement_matches_exact_rationals(inputs):
    """tests/_sens.py at 400 bits against the same algorithm in exact
    rationals of the float inputs, DMTM at 450 K / 1e4 Pa (condition 8e16 after
    row equilibration): equal to 1e-100; at 53 bits the algorithm is wrong in
    the third digit, which is why the kernel is double-double; the sum rule
    holds; and the fixture stores this answer."""
    import mpmath
    import _sens as S
    spec = O.load_spec(os.path.join(inputs, 'DMTM', 'input.json'))
    m = O.ClassicModel(spec, T=450.0, p=1e4)
    y, _ = m.solve_odes(rtol=1e-6, atol=1e-12)
    y = m.find_steady(y)
    assert m.regular
    exact, tof = S.adjoint_drc(m, y, ['r5', 'r9'], Fraction)
    assert abs(float(tof) - m.tof(y, ['r5', 'r9'])) <= 1e-9 * abs(float(tof))
    assert abs(float(sum(exact)) - 1.0) <= 1e-9
    x400, _ = S.adjoint_drc_mp(m, y, ['r5', 'r9'], 400)
    x53, _ = S.adjoint_drc_mp(m, y, ['r5', 'r9'], 53)
    with mpmath.workprec(1000):
        ex = [mpmath.mpf(a.numerator) / a.denominator for a in exact]
        assert max(abs(a - b) for a, b in zip(ex, x400)) <= mpmath.mpf(10) ** -100
        assert max(abs(a - b) for a, b in zip(ex, x53)) >= 1e-6
    fx = dict(np.load(os.path.join(HERE, 'golden', 'drc_adjoint_fixture.npz')))
    i = [str(x) for x in fx['names']].index('dmtm_450_10000')
    np.testing.assert_allclose(fx['c%d_y' % i], y[m.dyn], rtol=1e-9, atol=1e-30)
    np.testing.assert_allclose(fx['c%d_xi_ref' % i], [float(a) for a in exact], rtol=1e-6, atol=1e-9)
