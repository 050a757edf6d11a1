"""CPU-side checks of the adjoint sensitivities (reaction orders, apparent
activation energy, per-direction sensitivities): the C-ABI's two entry points
(pck_sens_at, pck_sens_adjoint), the kernel's code-object metadata, argument
checks that need no device and the arbitrary-precision restatement the GPU
tests are measured against (tests/_sens_ext.py)."""
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


def test_header_and_binding_abi_10():
    txt = open(os.path.join(ROOT, 'include', 'pycatkin_amd.h')).read()
    assert _lib.ABI_VERSION == 10 and '#define PCK_ABI_VERSION 10' in txt
    assert re.search(r'\bint pck_sens_at\(', txt) and re.search(r'\bint pck_sens_adjoint\(', txt)
    assert re.search(r'#define PCK_ST_SENS_PRECISION 8\b', txt) and _lib.ST_SENS_PRECISION == 8
    assert 'pck_sens_at' in _lib.EXPORTED and 'pck_sens_adjoint' in _lib.EXPORTED
    plain = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    for cname, pyname in (('pck_sens_out', 'SensOut'), ('pck_sens_dirs', 'SensDirs')):
        body = re.search(r'typedef struct \{([^{}]*)\}\s*%s;' % cname, plain).group(1)
        members = [d.replace('*', ' ').split()[-1] for decl in body.split(';') if decl.strip()
                   for d in decl.split(',')]
        assert members == [f[0] for f in getattr(_lib, pyname)._fields_], cname


def test_library_exports_the_entry_points():
    import ctypes
    import torch  # noqa: F401  (the library binds to torch's HIP runtime, pycatkin_amd/_lib.py)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('pck_sens_at', 'pck_sens_adjoint'):
        getattr(lib, name)
    lib.pck_abi_version.restype = ctypes.c_int
    assert lib.pck_abi_version() == 10


def test_wave_order_is_validated(inputs):
    """An invalid wave_order is a ValueError naming the argument, raised before
    anything is compiled or uploaded (it was a bare KeyError after the plan)."""
    import pycatkin_amd as P
    s = P.read_from_input_file(os.path.join(inputs, 'DMTM', 'input.json'))
    with pytest.raises(ValueError, match='wave_order'):
        s.solve_batch(T=[500.0], wave_order='bogus')


def test_sensitivity_batch_needs_a_steady_state(inputs):
    import pycatkin_amd as P
    s = P.read_from_input_file(os.path.join(inputs, 'DMTM', 'input.json'))
    with pytest.raises(ValueError, match='steady'):
        s.sensitivity_batch(('r5', 'r9'), T=[500.0], steady=False)
    with pytest.raises(ValueError, match='ss_solve'):
        s.reaction_orders(['r5', 'r9'], ss_solve=False)


def test_sens_kernels_use_no_scratch(tmp_path):
    """The code object's notes report private_segment_fixed_size == 0 for the
    three k_sens_adjoint<G> instances (the method of
    test_drc_adjoint.test_adjoint_kernels_use_no_scratch)."""
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
            if 'k_sens_adjoint' in name:
                found[name] = int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', b).group(1))
    assert len(found) == 3 and set(found.values()) == {0}, found


def _dmtm_450(inputs):
    spec = O.load_spec(os.path.join(inputs, 'DMTM', 'input.json'))
    m = O.ClassicModel(spec, T=450.0, p=1e4)
    fx = dict(np.load(os.path.join(HERE, 'golden', 'drc_adjoint_fixture.npz')))
    i = [str(x) for x in fx['names']].index('dmtm_450_10000')
    assert np.array_equal(m.kf, fx['c%d_kf' % i])
    return m, fx['c%d_y_full' % i], i


def test_restatement_matches_exact_rationals(inputs):
    """tests/_sens_ext.py at 400 bits against the same formulas in exact
    rationals of the float inputs, DMTM at 450 K / 1e4 Pa: every output equal
    to 1e-100 (relative to the largest of its kind); sf + sr = xi, xi is
    _sens.adjoint_drc's, and the fixture stores this answer."""
    import mpmath
    import _sens as S0
    import _sens_ext as S
    m, y, i = _dmtm_450(inputs)
    R = len(m.rnames)
    d = [(np.linspace(-1.0, 1.0, R), np.linspace(0.5, -0.25, R))]
    exact = S.adjoint_sens(m, y, ['r5', 'r9'], Fraction, directions=d)
    x400 = S.adjoint_sens_mp(m, y, ['r5', 'r9'], 400, directions=d)
    xi0, _ = S0.adjoint_drc(m, y, ['r5', 'r9'], Fraction)
    assert exact['xi'] == xi0
    assert all(a + b == c for a, b, c in zip(exact['sf'], exact['sr'], exact['xi']))
    assert len(exact['order']) == 3 and not exact['order_in']
    with mpmath.workprec(1000):
        q = lambda a: mpmath.mpf(a.numerator) / a.denominator
        for key in ('sf', 'sr', 'xi', 'dir'):
            big = max(abs(q(a)) for a in exact[key])
            assert max(abs(q(a) - b) for a, b in zip(exact[key], x400[key])) <= mpmath.mpf(10) ** -100 * big, key
        for k, a in exact['order'].items():
            assert abs(q(a) - x400['order'][k]) <= mpmath.mpf(10) ** -100
    fx = dict(np.load(os.path.join(HERE, 'golden', 'sensitivity_fixture.npz')))
    assert str(fx['names'][i]) == 'dmtm_450_10000'
    np.testing.assert_allclose(fx['c%d_sf_ref' % i], [float(a) for a in exact['sf']], rtol=1e-14, atol=1e-300)
    np.testing.assert_allclose(fx['c%d_order_ref' % i], [float(exact['order'][str(k)]) for k in fx['c%d_order_names' % i]],
                               rtol=1e-14, atol=1e-300)


def test_fp64_orders_miss(inputs):
    """Why the kernel is double-double: the DMTM reaction orders at 450 K are
    ~1e-6 and below, and the same formulas at 53 bits miss them by more than
    1e-7 absolute."""
    import _sens_ext as S
    m, y, _ = _dmtm_450(inputs)
    x400 = S.flat(S.adjoint_sens_mp(m, y, ['r5', 'r9'], 400))
    x53 = S.flat(S.adjoint_sens_mp(m, y, ['r5', 'r9'], 53))
    assert np.max(np.abs(x53['order'] - x400['order'])) > 1e-7
    assert np.max(np.abs(x400['order'])) < 1e-5


def test_fixture_guard_and_cases():
    """The fixture: 19 regular cases, 18 of them under the default guard
    (err <= 1e-9, the largest 7.4e-11), volcano_-2.5_0.5 far above it with a
    104-bit answer that is wrong by more than 1; the 104-bit run within err
    (+ one ulp of the double) of the 400-bit one everywhere."""
    fx = dict(np.load(os.path.join(HERE, 'golden', 'sensitivity_fixture.npz')))
    names = [str(x) for x in fx['names']]
    reg = [int(i) for i in fx['regular']]
    assert len(reg) == 19
    ok = [i for i in reg if float(fx['c%d_err' % i]) <= 1e-9]
    assert len(ok) == 18 and max(float(fx['c%d_err' % i]) for i in ok) < 1e-10
    bad = [i for i in reg if i not in ok]
    assert [names[i] for i in bad] == ['volcano_-2.5_0.5']
    assert float(fx['c%d_err' % bad[0]]) > 1.0 and np.max(np.abs(fx['c%d_order_104' % bad[0]] - fx['c%d_order_ref' % bad[0]])) > 1.0
    for i in reg:
        for key in ('sf', 'sr', 'order', 'order_in', 'dir'):
            a, b = fx['c%d_%s_104' % (i, key)], fx['c%d_%s_ref' % (i, key)]
            assert np.all(np.abs(a - b) <= float(fx['c%d_err' % i]) + 2.0 ** -51 * np.abs(b)), (names[i], key)
