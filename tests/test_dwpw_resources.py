"""Build check (CPU, hipcc -S, ~10 s): k_dwpw's register budget and the form of its depthwise loads.

The kernel runs at two waves per SIMD and is bound by the latency of a per-chunk dependent chain, so what a
change to it may not do is take registers: no instance that launch_dwpw can pick on the default path -- both matrix pipes --
may use more VGPRs than before the halo taps became range-checked buffer loads (the table below, from
profiles/r06_kernel_resources.txt), spill, or use scratch.  And the taps ARE buffer loads: from the head of the chunk loop to
the LDS writes of the depthwise tile a wave issues at least its 18 tap loads as buffer_load_dwordx4 and no global_load_dwordx4
(the depthwise weights and the bias come through resources of their own)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'retargetvid_amd', 'csrc')

# (NT, PW, MX) -> VGPRs of the parent (profiles/r06_kernel_resources.txt); NWV = 4 everywhere.  The instances of launch_dwpw's
# switch: 8-wide patches at NT = 2 .. 5 on both pipes, 16-wide patches (the 13-wide lowest level) at NT = 4 and 5, split-bf16 only.
PARENT_VGPRS = {(2, 8, 1): 208, (2, 8, 0): 210, (3, 8, 1): 226, (3, 8, 0): 232, (4, 8, 1): 244, (4, 8, 0): 252,
                (5, 8, 1): 256, (5, 8, 0): 256, (4, 16, 1): 244, (5, 16, 1): 256}


def _makefile_flags():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    arch = re.search(r'^ARCH\s*\?=\s*(\S+)', mk, re.M).group(1)
    flags = re.search(r'^CXXFLAGS\s*:=\s*(.*)$', mk, re.M).group(1).replace('$(ARCH)', arch).split()
    hipcc = re.search(r'^HIPCC\s*\?=\s*(\S+)', mk, re.M).group(1)
    return hipcc, flags


def _launchable(src):
    """The (NT, PW, MX) of every k_dwpw<...> that launch_dwpw names."""
    body = src[src.index('static int launch_dwpw('):]
    body = body[:body.index('\n}\n')]
    got = set()
    for nt, pw, nwv, mx in re.findall(r'k_dwpw<(\d), (\d+), (\d)(, true)?>', body):
        assert nwv == '4'
        got.add((int(nt), int(pw), 1 if mx else 0))
    return got


def test_dwpw_instances_keep_their_registers_and_load_taps_through_buffers():
    hipcc, flags = _makefile_flags()
    assert '--offload-arch=gfx950' in flags
    src = open(os.path.join(CSRC, 'svc_net.hip')).read()
    assert _launchable(src) == set(PARENT_VGPRS)
    asm = subprocess.run([hipcc] + flags + ['-S', '--cuda-device-only', '-o', '-', os.path.join(CSRC, 'svc_net.hip')],
                         capture_output=True, text=True, check=True).stdout
    entries = re.split(r'\n  - ', asm[asm.index('amdhsa.kernels:'):])
    seen = set()
    for (nt, pw, mx), parent in sorted(PARENT_VGPRS.items()):
        name = '_Z6k_dwpwILi%dELi%dELi4ELb%dEE' % (nt, pw, mx)
        mine = [e for e in entries if re.search(r'\.name:\s+%s\w*\s' % name, e)]
        assert len(mine) == 1, name
        meta = {k: int(v) for k, v in re.findall(r'\.(\w+):\s+(\d+)\s', mine[0])}
        print('k_dwpw<%d, %d, 4, %d>: %d VGPRs (parent %d, %d spilled), %d SGPRs (%d spilled), %d B scratch' % (
            nt, pw, mx, meta['vgpr_count'], parent, meta['vgpr_spill_count'], meta['sgpr_count'], meta['sgpr_spill_count'],
            meta['private_segment_fixed_size']))
        assert meta['vgpr_count'] <= parent, (nt, pw, mx)
        assert meta['vgpr_spill_count'] == 0 and meta['sgpr_spill_count'] == 0 and meta['private_segment_fixed_size'] == 0, (nt, pw, mx)
        # the function body: label .. s_endpgm.  The chunk loop's head is the last block label before the first buffer load;
        # the depthwise tile is parked by the first ds_write_b128 after it.
        start = asm.index('\n%s' % re.search(r'\.name:\s+(\S+)', mine[0]).group(1) + ':')
        body = asm[start:asm.index('s_endpgm', start)]
        first = body.index('buffer_load_dwordx4')
        head = max(m.start() for m in re.finditer(r'^\.LBB\d+_\d+:', body[:first], re.M))
        park = body.index('ds_write_b128', first)
        dw = body[head:park]
        print('   chunk head .. tile parked: %d buffer_load_dwordx4, %d global_load_dwordx4' % (
            dw.count('buffer_load_dwordx4'), dw.count('global_load_dwordx4')))
        assert dw.count('buffer_load_dwordx4') >= 18, (nt, pw, mx)
        assert dw.count('global_load_dwordx4') == 0, (nt, pw, mx)
        seen.add((nt, pw, mx))
    assert seen == set(PARENT_VGPRS)
