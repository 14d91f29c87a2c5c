"""Build check (CPU, hipcc -S, ~10 s): how k_pwr and k_smooth_down_mfma stage their operands, and what it costs in registers.

Both kernels bring operands to LDS in front of their first barrier.  Written as a loop of "load a piece, store it", hipcc compiles
the staging to one global load per iteration with an s_waitcnt vmcnt(0) on it -- 6 to 15 dependent round trips in k_pwr, 21 in
k_smooth_down_mfma -- so the requests are explicit (ld16_issue / ld16_wait in svc_net.hip) and this test reads the assembly:

* every k_pwr instance launch_pw_ex can pick, on both matrix pipes, and k_smooth_down_mfma: no spill, no scratch, and no more VGPRs
  than keep the waves per SIMD of the parent's build (profiles/r06_kernel_resources.txt) at the workgroups per CU the kernel's LDS
  request allows (160 KB per CU; a workgroup is one wave on each of the four SIMDs);
* from the kernel's entry to its first barrier no basic block branches to itself with a global load and a wait for it inside;
* the staged loads are ONE run in front of the first wait: the thread's pieces of the weight chunk (64 rows of C pieces over 256
  threads) and the wave's activations (K / 8 per lane) in k_pwr, four pieces of the logits and four of the phase table in
  k_smooth_down_mfma -- and that first wait leaves all the others in flight (vmcnt(run - 1))."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'retargetvid_amd', 'csrc')

# (KS, UPS, MX) -> VGPRs of the parent (profiles/r06_kernel_resources.txt)
PARENT_VGPRS = {(8, 1, 1): 224, (8, 0, 1): 94, (8, 1, 0): 206, (8, 0, 0): 74, (12, 0, 1): 126, (12, 0, 0): 90,
                (16, 1, 1): 256, (16, 0, 1): 142, (16, 1, 0): 238, (16, 0, 0): 102, (20, 0, 1): 166, (20, 0, 0): 122}
PARENT_SMOOTH_VGPRS = 95 + 16           # architectural + accumulation registers
SMOOTH = '_Z18k_smooth_down_mfma'
CU_LDS = 160 * 1024
PWR_NT, PWR_SLAB = 2, 36


def _makefile_flags():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    arch = re.search(r'^ARCH\s*\?=\s*(\S+)', mk, re.M).group(1)
    flags = re.search(r'^CXXFLAGS\s*:=\s*(.*)$', mk, re.M).group(1).replace('$(ARCH)', arch).split()
    hipcc = re.search(r'^HIPCC\s*\?=\s*(\S+)', mk, re.M).group(1)
    return hipcc, flags


def launchable(src):
    """The (KS, UPS) of every k_pwr instance launch_pw_ex names; it takes either pipe's."""
    body = src[src.index('static int launch_pw_ex('):]
    body = body[:body.index('\n}\n')]
    return {(int(ks), 1 if ups == 'true' else 0) for ks, ups in re.findall(r'pwr_kfn<(\d+), (true|false)>', body)}


def waves_by_vgprs(v):
    return min(8, 512 // (-(-v // 8) * 8))


def pwr_lds(K, mx):
    """launch_pw_ex's request at ntw = PWR_NT."""
    chunk = PWR_NT * 32 * ((K // 16) * 6 + 1) * 16 if mx else PWR_NT * 32 * (K + 4) * 4
    return chunk + (4 * 32 * PWR_SLAB + 128) * 4


def vgpr_cap(parent, lds):
    """The most VGPRs that keep the parent's waves per SIMD where the LDS request (None: not the limit) lets them run."""
    waves = waves_by_vgprs(parent) if lds is None else min(waves_by_vgprs(parent), CU_LDS // lds)
    return 512 // waves // 8 * 8


def kernel(asm, prefix):
    """(metadata, body up to s_endpgm) of the one kernel whose symbol starts with `prefix`."""
    entries = re.split(r'\n  - ', asm[asm.index('amdhsa.kernels:'):])
    mine = [e for e in entries if re.search(r'\.name:\s+%s\w*\s' % re.escape(prefix), e)]
    assert len(mine) == 1, prefix
    meta = {k: int(v) for k, v in re.findall(r'\.(\w+):\s+(\d+)\s', mine[0])}
    start = asm.index('\n%s:' % re.search(r'\.name:\s+(\S+)', mine[0]).group(1))
    return meta, asm[start:asm.index('s_endpgm', start)]


def prologue(body):
    """Entry .. first barrier (k_smooth_down_mfma carries SVC_NO_PK, its barriers are calls)."""
    ends = [m.start() for m in re.finditer(r'^\s*(s_barrier|s_swappc_b64)\b', body, re.M)]
    assert ends, 'no barrier'
    return body[:ends[0]]


def self_waiting_loops(pro):
    """Labels of the basic blocks that branch to themselves and hold a global load with a wait for every load behind it."""
    bad = []
    blocks = re.split(r'^(\.LBB\d+_\d+):', pro, flags=re.M)
    for label, text in zip(blocks[1::2], blocks[2::2]):
        loops = re.search(r'^\s*s_cbranch_\w+\s+%s\s*$' % re.escape(label), text, re.M)
        load = re.search(r'^\s*(global|buffer)_load_', text, re.M)
        if loops and load and re.search(r's_waitcnt[^\n]*vmcnt\(0\)', text[load.end():]):
            bad.append(label)
    return bad


def first_run(pro):
    """(16-byte global loads in front of the first wait on vector memory, that wait's count)."""
    w = re.search(r's_waitcnt[^\n]*vmcnt\((\d+)\)', pro)
    assert w, 'no wait'
    return len(re.findall(r'^\s*global_load_dwordx4\b', pro[:w.start()], re.M)), int(w.group(1))


def check(asm, instances):
    for (ks, ups, mx) in sorted(instances):
        K = 8 * ks
        name = '_Z5k_pwrILi%dELb%dELb%dEE' % (ks, ups, mx)
        meta, body = kernel(asm, name)
        cap = vgpr_cap(PARENT_VGPRS[(ks, ups, mx)], pwr_lds(K, mx))
        pro = prologue(body)
        run, count = first_run(pro)
        pieces = (K // 16) * 6 if mx else K // 4
        want = -(-PWR_NT * 32 * pieces // 256) + ks
        print('k_pwr<%d, %d, %d>: %d VGPRs (parent %d, cap %d, %d spilled), %d SGPRs spilled, %d B scratch; %d loads in front of vmcnt(%d), %d staged'
              % (ks, ups, mx, meta['vgpr_count'], PARENT_VGPRS[(ks, ups, mx)], cap, meta['vgpr_spill_count'], meta['sgpr_spill_count'],
                 meta['private_segment_fixed_size'], run, count, want))
        assert meta['vgpr_count'] <= cap, (ks, ups, mx)
        assert meta['vgpr_spill_count'] == 0 and meta['sgpr_spill_count'] == 0 and meta['private_segment_fixed_size'] == 0, (ks, ups, mx)
        assert not self_waiting_loops(pro), (ks, ups, mx, self_waiting_loops(pro))
        assert run >= want and count == run - 1, (ks, ups, mx, run, count, want)
    meta, body = kernel(asm, SMOOTH)
    pro = prologue(body)
    run, count = first_run(pro)
    cap = vgpr_cap(PARENT_SMOOTH_VGPRS, None)
    print('k_smooth_down_mfma: %d VGPRs (parent %d, cap %d, %d spilled), %d SGPRs spilled, %d B scratch; %d loads in front of vmcnt(%d)'
          % (meta['vgpr_count'], PARENT_SMOOTH_VGPRS, cap, meta['vgpr_spill_count'], meta['sgpr_spill_count'], meta['private_segment_fixed_size'],
             run, count))
    assert meta['vgpr_count'] <= cap
    assert meta['vgpr_spill_count'] == 0 and meta['sgpr_spill_count'] == 0 and meta['private_segment_fixed_size'] == 0
    assert not self_waiting_loops(pro), self_waiting_loops(pro)
    assert run >= 8 and count == run - 1, (run, count)


@pytest.fixture(scope='module')
def assembly():
    hipcc, flags = _makefile_flags()
    assert '--offload-arch=gfx950' in flags
    return subprocess.run([hipcc] + flags + ['-S', '--cuda-device-only', '-o', '-', os.path.join(CSRC, 'svc_net.hip')],
                          capture_output=True, text=True, check=True).stdout


def test_staging_requests_everything_before_the_first_wait_and_keeps_the_register_brackets(assembly):
    src = open(os.path.join(CSRC, 'svc_net.hip')).read()
    assert re.search(r'^#define PWR_NT %d$' % PWR_NT, src, re.M) and re.search(r'^#define PWR_SLAB %d\b' % PWR_SLAB, src, re.M)
    picks = launchable(src)
    instances = {(ks, ups, mx) for ks, ups in picks for mx in (0, 1)}
    assert instances == set(PARENT_VGPRS), sorted(instances)
    check(assembly, instances)


def test_the_checks_see_a_piece_by_piece_loop():
    """The form the staging had: what self_waiting_loops and first_run make of it."""
    pro = ('\ts_cbranch_execz .LBB0_3\n.LBB0_2:\n\tglobal_load_dwordx4 v[6:9], v[6:7], off\n\tv_add_u32_e32 v1, 0x100, v1\n'
           '\ts_waitcnt vmcnt(0)\n\tds_write_b128 v5, v[6:9]\n\ts_cbranch_execnz .LBB0_2\n.LBB0_3:\n')
    assert self_waiting_loops(pro) == ['.LBB0_2']
    assert first_run(pro) == (1, 0)
