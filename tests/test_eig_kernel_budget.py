"""Resource report of the eigenvalue kernels (no GPU): csrc/tu_eig.hip compiled
device-only with the build's flags and the compiler's resource-usage remarks.
k_eig_lane and k_eig_grp<16 | 32 | 64> keep every run-time indexed array in LDS:
no kernel may use scratch or spill (DESIGN.md "Linear stability": 94 VGPRs and
5 waves per SIMD for the one-lane kernel, 104 to 108 and 4 for the group
kernels)."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as G

SRC = os.path.join(G.ROOT, 'pycatkin_amd', 'csrc', 'tu_eig.hip')


@pytest.fixture(scope='module')
def usage(tmp_path_factory):
    """{kernel name: {remark field: value}} of every kernel in the unit."""
    out = tmp_path_factory.mktemp('eig_budget') / 'tu_eig.o'
    cmd = ([G.HIPCC] + G.HIPFLAGS + G.SPLIT + ['-I' + os.path.join(G.ROOT, 'include'), '--cuda-device-only',
                                                '-Rpass-analysis=kernel-resource-usage', '-c', '-o', str(out), SRC])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    kernels, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r'remark:\s+(.*?)\s*\[-Rpass-analysis', line)
        if not m:
            continue
        text = m.group(1)
        if text.startswith('Function Name:'):
            cur = kernels.setdefault(text.split(':', 1)[1].strip(), {})
        elif cur is not None and ':' in text:
            key, val = text.rsplit(':', 1)
            cur[key.strip()] = val.strip()
    return kernels


@pytest.mark.parametrize('stem', ['k_eig_laneE', 'k_eig_grpILi16E', 'k_eig_grpILi32E', 'k_eig_grpILi64E', 'k_eig_reduce'])
def test_eig_kernel_has_no_scratch(usage, stem):
    ks = {k: v for k, v in usage.items() if stem in k}
    assert len(ks) == 1, (stem, sorted(usage))
    (name, u), = ks.items()
    print(name, u)
    assert int(u['ScratchSize [bytes/lane]']) == 0, (name, u)
    assert int(u['VGPRs Spill']) == 0 and int(u['SGPRs Spill']) == 0, (name, u)
    assert int(u['Occupancy [waves/SIMD]']) >= 4, (name, u)
