"""DevBuf (retargetvid_amd/csrc/svc_devbuf.h) owns its device memory: tests/native/devbuf_harness.cpp, a program of its own
over counting stubs of hipMalloc / hipFree, built with the address and undefined-behaviour sanitizers (leak detection
included) and run as a child process.  It walks ensure growth, moves, self-move, the map and pair shapes of the handle's
cached tables and the early returns that used to leak; its static_asserts state that DevBuf and ResampleTab cannot be
copied.  No GPU, no HIP runtime."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INCLUDE = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'include')


def test_devbuf_ownership_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'devbuf_harness')
    # the sanitizer runtimes linked into the program itself: it runs as it is, whatever else the process environment loads
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-static-libasan', '-static-libubsan',
                           '-D__HIP_PLATFORM_AMD__', '-I' + HIP_INCLUDE, '-o', exe,
                           os.path.join(ROOT, 'tests', 'native', 'devbuf_harness.cpp')])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1')
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == '', r.stderr                         # a sanitizer reports on stderr; UBSan alone would not change the status
    assert r.stdout.startswith('devbuf_harness ok')
