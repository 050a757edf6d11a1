"""Energy landscapes without a GPU: the loader, the symbolic landscape forms,
the C-ABI mirrors of pck_energy_span and the span kernel's code object.
The numbers are checked on the device in test_gpu_energy_span.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pycatkin_amd as P
from pycatkin_amd import _lib
from pycatkin_amd.classes.energy import Energy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, 'include', 'pycatkin_amd.h')
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'energy_span_fixture.npz')
LLVM = '/opt/rocm/lib/llvm/bin'


@pytest.fixture(scope='module')
def dmtm(inputs):
    return P.read_from_input_file(os.path.join(inputs, 'DMTM', 'input.json'))


def test_loader_reads_energy_landscapes(dmtm):
    """load_input.py:154-163 and test/test_1.py step 3."""
    fx = np.load(FIXTURE)
    assert dmtm.energy_landscapes is not None
    assert list(dmtm.energy_landscapes) == ['full_pes']
    pes = dmtm.energy_landscapes['full_pes']
    assert isinstance(pes, Energy) and pes.name == 'full_pes'
    assert len(pes.minima) == 20
    assert pes.labels == [entry[0].name for entry in pes.minima]
    assert pes.minima[3][0] is dmtm.states['CuO2Cu'] and [s.name for s in pes.minima[3]] == ['CuO2Cu', 'CH4', 'CH4']
    assert pes.is_ts() == list(fx['dmtm_free_isTS'])
    assert pes.energy_landscape is None


def test_constructor_mirrors_the_reference(dmtm):
    a, b = dmtm.states['2Cu'], dmtm.states['TS1']
    assert Energy(minima=[[a], [b]]).labels == ['2Cu', 'TS1']
    assert Energy(name='x', minima=[[a], [b]], labels=['p', 'q']).labels == ['p', 'q']
    with pytest.raises(AssertionError):
        Energy(minima=[[a], [b]], labels=['only one'])
    with pytest.raises(NotImplementedError, match='pickle'):
        Energy(path_to_pickle='energy_landscape.pckl')
    with pytest.raises(NotImplementedError, match='pickle'):
        Energy(minima=[[a], [b]]).save_pickle()
    with pytest.warns(UserWarning, match='plotting'):
        Energy(minima=[[a], [b]]).draw_energy_landscape(T=400.0, p=1e5)


def _live(form):
    return {k: v for k, v in form.terms.items() if v != 0.0}


def test_landscape_forms_cancel_against_entry_0(dmtm):
    """Constants plus thermal features only; a state that an entry shares with
    entry 0 leaves no term behind."""
    pes = dmtm.energy_landscapes['full_pes']
    forms = pes.landscape_forms()
    ref = {s.name: pes.minima[0].count(s) for s in pes.minima[0]}
    assert len(forms['free']) == len(forms['electronic']) == 20
    assert _live(forms['free'][0]) == {} and _live(forms['electronic'][0]) == {}
    for k, entry in enumerate(pes.minima):
        assert set(_live(forms['electronic'][k])) <= {('1',)}
        live = _live(forms['free'][k])
        assert all(key == ('1',) or key[0] in ('vib', 'tran', 'rot') for key in live), live
        names = {s.name for s in entry} | set(ref)
        for name in names:
            net = sum(1 for s in entry if s.name == name) - ref.get(name, 0)
            # (an adsorbate's gasdata adds fractions of a gas state's tran / rot
            # features, so the whole-number count is checked on vib)
            assert live.get(('vib', name), 0.0) in (0.0, net), (k, name)
            if net == 0 and not any(s.gasdata for s in entry):
                assert not any(key[1:] == (name,) for key in live), (k, name)
    # entry 19 closes the cycle: 2 CH3OH made from O2 and 2 CH4, the sites cancel
    assert {key[1] for key in _live(forms['free'][19]) if key != ('1',)} == {'CH3OH', 'O2', 'CH4'}


def test_energy_modifier_reaches_free_forms_only(inputs):
    sim = P.read_from_input_file(os.path.join(inputs, 'DMTM', 'input.json'))
    pes = sim.energy_landscapes['full_pes']
    key0 = tuple(repr(f) for f in pes.landscape_forms()['free'])
    sim.states['TS3'].set_energy_modifier(P.Descriptor('x'))
    forms = pes.landscape_forms()
    for k, entry in enumerate(pes.minima):
        has = 'TS3' in [s.name for s in entry]
        assert _live(forms['free'][k]).get(('desc', 'x'), 0.0) == (1.0 if has else 0.0)
        assert ('desc', 'x') not in _live(forms['electronic'][k])
    # the plan cache is keyed on the forms: the modifier changes the key
    assert tuple(repr(f) for f in forms['free']) != key0
    # a modifier on a state of entry 0 shifts every other entry
    sim.states['2Cu'].set_energy_modifier(P.Descriptor('y'))
    forms = pes.landscape_forms()
    assert _live(forms['free'][0]) == {}
    assert _live(forms['free'][5]).get(('desc', 'y')) == -1.0
    assert ('desc', 'y') not in _live(forms['free'][19])


def _struct_fields(txt, name):
    """Member names of `typedef struct { ... } name;` in declaration order
    (array bounds dropped)."""
    body = re.search(r"typedef struct \{([^{}]*)\}\s*%s;" % name, txt).group(1)
    out = []
    for decl in body.split(';'):
        decl = re.sub(r'\[[^\]]*\]', '', decl).strip()
        if not decl:
            continue
        first, *rest = [d.strip() for d in decl.split(',')]
        out.append(first.replace('*', ' ').split()[-1])
        out += [r.replace('*', ' ').split()[-1] for r in rest]
    return out


@pytest.mark.parametrize('cname, pyname', [('pck_landscape', 'Landscape'), ('pck_span_outputs', 'SpanOutputs')])
def test_span_struct_layouts_match_header(cname, pyname):
    txt = re.sub(r'/\*.*?\*/', '', open(HDR).read(), flags=re.S)
    assert _struct_fields(txt, cname) == [f[0] for f in getattr(_lib, pyname)._fields_]


def test_span_abi_constants():
    import ctypes
    txt = open(HDR).read()
    assert '#define PCK_MAX_PES %d' % _lib.MAX_PES in txt
    assert _lib.ABI_VERSION >= 7 and 'pck_energy_span' in _lib.EXPORTED
    assert ctypes.sizeof(_lib.Landscape) == 4 + 4 * _lib.MAX_PES + 4 + 8     # n_pts, reg, padding, ts_mask
    from pycatkin_amd.engine import DeviceNetwork
    assert set(f[0] for f in _lib.SpanOutputs._fields_) - {'ld_x', 'ld_e'} == set(DeviceNetwork.SPAN_OUTPUTS)


@pytest.mark.skipif(not (os.path.isfile(_lib.LIB_PATH) and os.path.isfile(LLVM + '/llvm-readelf')),
                    reason='library or ROCm LLVM tools absent')
def test_span_kernel_uses_no_scratch(tmp_path):
    """The per-lane arrays of run-time length live in the lane's LDS column:
    the code object's note reports private_segment_fixed_size == 0."""
    cp, fb, elf = str(tmp_path / 'lib_copy.so'), str(tmp_path / 'fb.bin'), str(tmp_path / 'k.elf')
    shutil.copyfile(_lib.LIB_PATH, cp)
    subprocess.run(['objcopy', '--dump-section', '.hip_fatbin=' + fb, cp], check=True)
    blob = open(fb, 'rb').read()
    starts = [m.start() for m in re.finditer(re.escape(b'__CLANG_OFFLOAD_BUNDLE__'), blob)]
    assert starts, 'no offload bundle in the library'
    found = []
    for i, a in enumerate(starts):
        part = str(tmp_path / ('fb%d.bin' % i))
        open(part, 'wb').write(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        subprocess.run([LLVM + '/clang-offload-bundler', '--type=o', '--input=' + part,
                        '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--output=' + elf, '--unbundle'], check=True)
        notes = subprocess.run([LLVM + '/llvm-readelf', '--notes', elf], check=True, capture_output=True,
                               text=True).stdout
        for b in notes.split('  - .agpr_count:')[1:]:
            if 'k_energy_span' in re.search(r'\.name:\s+(\S+)', b).group(1):
                found.append(int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', b).group(1)))
    assert found == [0], found
