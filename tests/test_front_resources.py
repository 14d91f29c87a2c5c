"""Build check (CPU, hipcc -S, ~10 s): k_front's occupancy budget.

The kernel is laid out for FOUR workgroups of 256 threads per CU (svc_net.hip, "LDS (round 4)"): that needs at most 128
VGPRs per lane, no scratch (a spill would be a trip to memory inside the resampling loops), and a dynamic LDS request of
which four fit in the CU's 160 KiB.  The register figures come from the kernel's metadata in the device assembly, compiled
with the Makefile's flags; the LDS request from the constants front_lds_bytes() is made of."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'retargetvid_amd', 'csrc')
LDS_PER_CU = 160 * 1024


def _makefile_flags():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    arch = re.search(r'^ARCH\s*\?=\s*(\S+)', mk, re.M).group(1)
    flags = re.search(r'^CXXFLAGS\s*:=\s*(.*)$', mk, re.M).group(1).replace('$(ARCH)', arch).split()
    hipcc = re.search(r'^HIPCC\s*\?=\s*(\S+)', mk, re.M).group(1)
    return hipcc, flags


def _define(src, name):
    """The integer value of `#define name <expression of numbers and earlier defines>`."""
    expr = re.search(r'^#define %s\s+(.*?)\s*(?://.*)?$' % name, src, re.M).group(1)
    expr = re.sub(r'[A-Z_][A-Z_0-9]*', lambda m: str(_define(src, m.group(0))), expr)
    assert re.fullmatch(r'[\d\s()+*/-]+', expr), (name, expr)
    return int(eval(expr))


def test_front_kernel_keeps_four_workgroups_per_cu():
    hipcc, flags = _makefile_flags()
    assert '--offload-arch=gfx950' in flags
    asm = subprocess.run([hipcc] + flags + ['-S', '--cuda-device-only', '-o', '-', os.path.join(CSRC, 'svc_net.hip')],
                         capture_output=True, text=True, check=True).stdout
    entries = [e for e in re.split(r'\n  - ', asm[asm.index('amdhsa.kernels:'):]) if re.search(r'\.name:\s+_Z7k_front9FrontArgs\s', e)]
    assert len(entries) == 1
    meta = {k: int(v) for k, v in re.findall(r'\.(\w+):\s+(\d+)\s', entries[0])}
    print('k_front: %d VGPRs (%d spilled), %d SGPRs (%d spilled), %d B scratch, %d B static LDS' % (
        meta['vgpr_count'], meta['vgpr_spill_count'], meta['sgpr_count'], meta['sgpr_spill_count'],
        meta['private_segment_fixed_size'], meta['group_segment_fixed_size']))
    assert meta['vgpr_count'] <= 128
    assert meta['vgpr_spill_count'] == 0 and meta['sgpr_spill_count'] == 0 and meta['private_segment_fixed_size'] == 0
    assert meta['max_flat_workgroup_size'] == 256
    # the dynamic LDS request: front_lds_bytes() = FR_IN_BYTES + FR_SONLY_BYTES, and nothing static beside it
    src = open(os.path.join(CSRC, 'svc_net.hip')).read()
    assert re.search(r'front_lds_bytes\(\)\s*\{\s*return FR_IN_BYTES \+ FR_SONLY_BYTES;\s*\}', src)
    assert re.search(r'k_front<<<[^;]*, 256, front_lds_bytes\(\), s>>>', src)
    lds = _define(src, 'FR_IN_BYTES') + _define(src, 'FR_SONLY_BYTES')
    assert lds == 21 * 112 * 4 + 180 * 36 * 4
    assert meta['group_segment_fixed_size'] == 0
    assert 4 * lds <= LDS_PER_CU
