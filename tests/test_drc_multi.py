"""CPU-side checks of the multi-objective analytic degree of rate control: the
C-ABI's two entry points (pck_drc_multi_at, pck_drc_multi_adjoint), the
kernels' code-object metadata, the arbitrary-precision restatement the GPU
tests are measured against (tests/_sens_multi.py), the fixture, and the
parsing of objectives, which needs no device."""
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
    assert re.search(r'\bint pck_drc_multi_at\(', txt) and re.search(r'\bint pck_drc_multi_adjoint\(', txt)
    assert 'pck_drc_multi_at' in _lib.EXPORTED and 'pck_drc_multi_adjoint' in _lib.EXPORTED
    plain = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    for cname, pyname in (('pck_multi_obj', 'MultiObj'), ('pck_multi_out', 'MultiOut')):
        body = re.search(r'typedef struct \{([^{}]*)\}\s*%s;' % cname, plain).group(1)
        members = [d.replace('*', ' ').split()[-1] for decl in body.split(';') if decl.strip()
                   for d in decl.split(',')]
        assert members == [f[0] for f in getattr(_lib, pyname)._fields_], cname


def test_library_exports_the_entry_points():
    import ctypes
    import torch  # noqa: F401  (the library binds to torch's HIP runtime, pycatkin_amd/_lib.py)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('pck_drc_multi_at', 'pck_drc_multi_adjoint'):
        getattr(lib, name)
    lib.pck_abi_version.restype = ctypes.c_int
    assert lib.pck_abi_version() == 10


def test_multi_kernels_use_no_scratch(tmp_path):
    """The code object's notes list exactly three k_multi_adjoint<G> instances,
    each with private_segment_fixed_size == 0 (the method of
    test_sensitivities.test_sens_kernels_use_no_scratch: metadata only)."""
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
            if 'k_multi_adjoint' in name:
                assert 'k_drc_adjoint' not in name and 'k_sens_adjoint' not in name
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
    """tests/_sens_multi.py at 400 bits against the same formulas in exact
    rationals of the float inputs, DMTM at 450 K / 1e4 Pa, for a rate
    objective (the TOF terms), a coverage and a weighted mix: every xi equal to
    1e-100 of the objective's largest, the values to 1e-100 relative; the TOF
    objective is _sens.adjoint_drc's answer exactly, and the mix obeys
    J_mix xi_mix = J_a xi_a + J_b xi_b exactly."""
    import mpmath
    import _sens as S0
    import _sens_multi as S
    m, y, _ = _dmtm_450(inputs)
    rn, dyn = list(m.rnames), [m.snames[q] for q in m.dyn]
    R, NS = len(rn), len(dyn)
    wr0, wy1 = np.zeros(R), np.zeros(NS)
    wr0[[rn.index('r5'), rn.index('r9')]] = 1.0
    wy1[dyn.index('sCH3OH')] = 1.0
    objs = [(wr0, np.zeros(NS)), (np.zeros(R), wy1), (2.5 * wr0, -0.5 * wy1)]
    exact, vex = S.multi_drc(m, y, objs, Fraction)
    x400, v400 = S.multi_drc_mp(m, y, objs, 400)
    xi0, tof0 = S0.adjoint_drc(m, y, ['r5', 'r9'], Fraction)
    assert exact[0] == xi0 and vex[0] == tof0
    assert vex[2] == Fraction(5, 2) * vex[0] - Fraction(1, 2) * vex[1]
    assert all(vex[2] * c == Fraction(5, 2) * vex[0] * a - Fraction(1, 2) * vex[1] * b
               for a, b, c in zip(*exact))
    with mpmath.workprec(1000):
        q = lambda a: mpmath.mpf(a.numerator) / a.denominator
        for k in range(3):
            big = max(abs(q(a)) for a in exact[k])
            assert max(abs(q(a) - b) for a, b in zip(exact[k], x400[k])) <= mpmath.mpf(10) ** -100 * big, k
            assert abs(q(vex[k]) - v400[k]) <= mpmath.mpf(10) ** -100 * abs(q(vex[k])), k


def test_fixture_cases_and_bounds():
    """The fixture: the twelve cases of the issue plus DMTM at 450 K with
    K = 22 objectives, at most 8 objectives elsewhere, every objective non-empty
    and its value non-zero, the 104-bit run within 1e-9 of the 400-bit one
    (the generator's condition), the finite difference of dmtm_600 within 1e-4;
    the TOF objective is drc_adjoint_fixture's xi_ref to 1e-14; the file is no
    larger than sensitivity_fixture.npz."""
    g = os.path.join(HERE, 'golden')
    fx, src = dict(np.load(os.path.join(g, 'drc_multi_fixture.npz'))), dict(np.load(os.path.join(g, 'drc_adjoint_fixture.npz')))
    names = [str(x) for x in fx['names']]
    want = ['dmtm_400_10000', 'dmtm_450_10000', 'dmtm_450_all', 'dmtm_600_100000', 'cstr_473', 'cstr_573',
            'volcano_-1_-1', 'volcano_-2.5_0.5', 'syn12_0', 'syn24_0', 'syn40_0', 'e64_0',
            'butadiene_with_jonas_byproducts_798']
    assert names == want
    assert os.path.getsize(os.path.join(g, 'drc_multi_fixture.npz')) <= os.path.getsize(os.path.join(g, 'sensitivity_fixture.npz'))
    for i, nm in enumerate(names):
        c = {k[len('m%d_' % i):]: v for k, v in fx.items() if k.startswith('m%d_' % i)}
        si = int(c['src'])
        K, R = c['xi_ref'].shape
        assert K == (22 if nm == 'dmtm_450_all' else len(c['labels'])) and (K <= 8 or nm == 'dmtm_450_all')
        assert c['wr'].shape == (K, R) and c['wy'].shape == (K, len(src['c%d_dyn' % si]))
        assert np.all(c['wr'].any(axis=1) | c['wy'].any(axis=1)) and np.all(c['val_ref'] != 0.0)
        assert np.all(np.isfinite(c['xi_ref'])) and np.all(np.isfinite(c['xi_pert']))
        assert np.max(np.abs(c['xi_104'] - c['xi_ref'])) <= 1e-9, nm
        if nm != 'dmtm_450_all':
            assert str(c['labels'][0]) == 'tof'
            np.testing.assert_allclose(c['xi_ref'][0], src['c%d_xi_ref' % si], rtol=1e-14, atol=1e-14)
            m, a, b = (int(v) for v in c['mix'])
            np.testing.assert_array_equal(c['wr'][m], c['wr'][a] + c['wr'][b])
            np.testing.assert_array_equal(c['wy'][m], c['wy'][a] + c['wy'][b])
        if nm == 'dmtm_600_100000':
            assert np.max(np.abs(c['xi_fd'] - c['xi_ref'])) <= 1e-4
        else:
            assert 'xi_fd' not in c


# ------------------------------------------------------------------ objectives are parsed on the host
def _dmtm(inputs):
    import pycatkin_amd as P
    return P.read_from_input_file(os.path.join(inputs, 'DMTM', 'input.json'))


def test_objectives_are_parsed_to_weights(inputs):
    """str -> one entry of wy; a tuple of reactions -> counts in wr (a name twice
    counts twice, as tof_terms counts it); a dict -> its weights.  The plan has
    no TOF terms."""
    s = _dmtm(inputs)
    plan = s.plan((), None)
    assert list(plan.tof_terms) == []
    labels, wr, wy = s._objectives(plan, ['sCH3OH', ('r5', 'r9', 'r9'), {'rates': {'r5': 2.5}, 'species': {'sO': -0.5}}])
    R, D = plan.reactions.index, plan.dyn.index
    assert wr.shape == (3, len(plan.reactions)) and wy.shape == (3, len(plan.dyn))
    assert wy[0, D('sCH3OH')] == 1.0 and wy[0].sum() == 1.0 and not wr[0].any()
    assert wr[1, R('r5')] == 1.0 and wr[1, R('r9')] == 2.0 and wr[1].sum() == 3.0 and not wy[1].any()
    assert wr[2, R('r5')] == 2.5 and wy[2, D('sO')] == -0.5
    assert labels[0] == 'sCH3OH' and labels[1] == 'r5+r9+r9'


@pytest.mark.parametrize('objectives,match', [
    (['nope'], "'nope' is an unknown species"),
    (['CH4'], "'CH4' is a fixed species"),
    ([('r5', 'r99')], "'r99' is an unknown reaction"),
    ([()], 'is empty'),
    ([{'rates': {'r5': 0.0}}], 'is empty'),
    ([{'rates': {'r5': 1.0}, 'specie': {}}], 'unknown keys'),
    ([{'species': {'CH4': 1.0}}], "'CH4' is a fixed species"),
    ([3.0], 'neither'),
    ([], 'no objectives'),
])
def test_bad_objectives_raise_before_any_device_work(inputs, objectives, match):
    """Unknown names, a fixed species and an empty objective are a ValueError
    naming the offender, raised before a network is uploaded: no device is
    needed to get it, from any of the entry points."""
    s = _dmtm(inputs)
    Y = np.zeros((len(s.plan((), None).dyn), 1))
    with pytest.raises(ValueError, match=match):
        s.drc_objectives_at(objectives, Y, T=[450.0], p=[1e4])
    with pytest.raises(ValueError, match=match):
        s.drc_objectives_batch(objectives, T=[450.0], p=[1e4])
    assert not any(v[1] is not None for v in s._plans.values())      # nothing was uploaded


def test_conveniences_check_their_names_on_the_host(inputs):
    s = _dmtm(inputs)
    with pytest.raises(ValueError, match="'r99' is an unknown reaction"):
        s.selectivity_control_batch(('r5',), ('r5', 'r99'), T=[450.0], p=[1e4])
    with pytest.raises(ValueError, match='is empty'):
        s.selectivity_control_batch(('r5',), (), T=[450.0], p=[1e4])
    with pytest.raises(ValueError, match="'O2' is a fixed species"):
        s.coverage_control_batch(['sO', 'O2'], T=[450.0], p=[1e4])
