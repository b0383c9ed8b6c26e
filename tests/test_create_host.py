"""CPU test: p3d_create on a machine without a device.  The first device allocation fails, so
every call goes through the create's one way out -- the memory owner's release on a partly filled
model -- and must answer P3D_ERR_HIP with the runtime's text, leave the handle null and leave the
process able to go on."""
import ctypes

import pytest
import torch

import _p3d

P3D_ERR_HIP = 2   # include/p3d.h


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a machine without a device")
def test_create_without_a_device_fails_cleanly_every_time():
    lib = _p3d.lib()
    cfg = _p3d.P3DCfg(1024, 2, 1, 1, 0, 32, 48, 0, 64, 1e-3, 0.99)   # cfg2
    for _ in range(50):
        h = ctypes.c_void_p()
        assert lib.p3d_create(ctypes.byref(cfg), ctypes.byref(h)) == P3D_ERR_HIP
        assert not h.value
        assert lib.p3d_last_error().startswith(b"p3d_create: ")
    assert lib.p3d_destroy(None) == 0
