"""CPU test of the active-row entry points' host side (include/mrcnn_hip.h: mrcnn_active_rows_u8, mrcnn_conv2d_bwd_data_active_f32,
mrcnn_conv2d_bwd_filter_active_f32): the stand-alone driver tests/native/active_rows_host_check.cpp against the library's host code
built with AddressSanitizer, like tests/test_abi_cpu.py::test_host_side_under_address_sanitizer (the same `make asan`)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_active_row_entry_points_reject_bad_arguments_under_address_sanitizer():
    if not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('hipcc not available')
    import torch
    if torch.cuda.device_count() > 0:       # (does not initialise the device)
        pytest.skip('host-only check: the driver passes null buffers on purpose and must not run where a GPU could execute a launch')
    csrc = os.path.join(ROOT, 'chainer-maskrcnn_amd', 'csrc')
    subprocess.check_call(['make', '-C', csrc, 'asan', '-j8'], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    rt = subprocess.check_output(['/opt/rocm/lib/llvm/bin/clang', '-print-file-name=libclang_rt.asan-x86_64.so']).decode().strip()
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0',
               LD_LIBRARY_PATH=os.path.dirname(rt) + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([os.path.join(csrc, 'asan', 'active_rows_host_check')], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0 and 'AddressSanitizer' not in out and ' 0 failure(s)' in out, out[-3000:]


def test_switch_defaults_on_and_bindings_know_the_entry_points():
    from chainer_maskrcnn import _hip
    from chainer_maskrcnn.nn import core
    assert core.MASK_BWD_SKIP_INACTIVE is True
    for name in ('mrcnn_active_rows_u8', 'mrcnn_conv2d_bwd_data_active_f32', 'mrcnn_conv2d_bwd_filter_active_f32'):
        assert name in _hip.SIGNATURES and hasattr(_hip.lib(), name)
