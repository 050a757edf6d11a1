"""Register budget of the compiled-in lane kernels (no GPU): csrc/tu_lane_ct.hip
compiled device-only with the build's flags and the compiler's resource-usage
remarks.  The volcano kernel must keep three waves per SIMD and no kernel may
spill to scratch (DESIGN.md "Lane step chain": the one-block stage sequence
can raise register pressure under max-ilp scheduling; the volcano kernel
stands at 163 VGPRs, the CSTR kernels at 255)."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as G

SRC = os.path.join(G.ROOT, 'pycatkin_amd', 'csrc', 'tu_lane_ct.hip')


@pytest.fixture(scope='module')
def usage(tmp_path_factory):
    """{kernel name: {remark field: value}} of every kernel in the unit."""
    out = tmp_path_factory.mktemp('lane_budget') / 'tu_lane_ct.o'
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


def _solve_kernels(usage, net):
    return {k: v for k, v in usage.items() if 'k_solve' in k and net in k}


def test_volcano_kernel_keeps_three_waves_and_no_scratch(usage):
    ks = _solve_kernels(usage, 'Volcano')
    assert ks, sorted(usage)
    for name, u in ks.items():
        print(name, u)
        assert int(u['Occupancy [waves/SIMD]']) == 3, (name, u)
        assert int(u['VGPRs']) <= 168, (name, u)
        assert int(u['ScratchSize [bytes/lane]']) == 0, (name, u)
        assert int(u['VGPRs Spill']) == 0, (name, u)


def test_cstr_kernels_have_no_scratch(usage):
    ks = _solve_kernels(usage, 'Cstr')
    assert len(ks) >= 2, sorted(usage)
    for name, u in ks.items():
        print(name, u)
        assert int(u['ScratchSize [bytes/lane]']) == 0, (name, u)
        assert int(u['VGPRs Spill']) == 0, (name, u)
