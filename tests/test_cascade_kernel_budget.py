"""Resource guard of the reactor-cascade kernels (csrc/mk_cascade.h), read
from the built library's gfx950 code object with the ROCm LLVM tools (no GPU).
Own copy of tests/test_capi.py's metadata reader."""
import os
import re
import shutil
import subprocess

import pytest

from pycatkin_amd import _lib

LLVM = '/opt/rocm/lib/llvm/bin'


def _kernel_metadata(lib_path, tmp_path):
    """name -> (vgpr_count, agpr_count, private_segment_fixed_size) of every
    kernel in the library's gfx950 code object."""
    fb, elf = str(tmp_path / 'fb.bin'), str(tmp_path / 'k.elf')
    # objcopy with no output file rewrites its input in place: work on a copy
    cp = str(tmp_path / 'lib_copy.so')
    shutil.copyfile(lib_path, cp)
    subprocess.run(['objcopy', '--dump-section', '.hip_fatbin=' + fb, cp], check=True)
    blob = open(fb, 'rb').read()
    magic = b'__CLANG_OFFLOAD_BUNDLE__'
    starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
    assert starts, 'no offload bundle in the library'
    notes = ''
    for i, a in enumerate(starts):
        part = str(tmp_path / ('fb%d.bin' % i))
        open(part, 'wb').write(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        subprocess.run([LLVM + '/clang-offload-bundler', '--type=o', '--input=' + part,
                        '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--output=' + elf, '--unbundle'], check=True)
        notes += subprocess.run([LLVM + '/llvm-readelf', '--notes', elf], check=True, capture_output=True,
                                text=True).stdout
    out = {}
    for b in notes.split('  - .agpr_count:')[1:]:
        g = lambda k: int(re.search(r'\.' + k + r':\s+(\d+)', b).group(1))
        out[re.search(r'\.name:\s+(\S+)', b).group(1)] = (g('vgpr_count'), int(b.split('\n')[0]),
                                                          g('private_segment_fixed_size'))
    return out


@pytest.mark.skipif(not (os.path.isfile(_lib.LIB_PATH) and os.path.isfile(LLVM + '/llvm-readelf')),
                    reason='library or ROCm LLVM tools absent')
def test_cascade_register_budget(tmp_path):
    """The cascade kernels over the compiled-in CSTR plans use no scratch (the
    shipped figure, DESIGN.md "Reactor cascade": 256 VGPRs + 60 AGPRs, 0 B);
    the runtime plans are exempt as for k_solve.  The library holds the ten
    instances: PlanRT<1..8> and the two CSTR plans."""
    md = _kernel_metadata(_lib.LIB_PATH, tmp_path)
    cas = {k: v for k, v in md.items() if 'k_cascade' in k}
    assert len(cas) == 10, sorted(cas)
    ct = {k: v for k, v in cas.items() if 'PlanRT' not in k}
    assert len(ct) == 2 and all('Cstr' in k for k in ct), sorted(ct)
    for k, (vg, ag, priv) in ct.items():
        assert priv == 0, (k, priv)
    # adding the cascade did not touch the solver's own budget
    for k, (vg, ag, priv) in md.items():
        if 'k_solve' in k and 'PlanRT' not in k:
            assert priv == 0, (k, priv)
