"""TEST INFRASTRUCTURE: builder and driver of the probe entry points (tests/devprobe/probes.inc) on both backends.

`build()` compiles tests/devprobe/devprobe.hip for gfx950 with the library's own flag list (contour-context_amd:
HIPCC_FLAGS) into tests/devprobe/libcc_devprobe.so; `GpuProbe` drives it with torch-allocated device memory, `EmuProbe`
drives the same probe_* entry points of the CPU harness (tests/emu/libcc_emu.so) with numpy memory.  Both have the same
three calls, so a case of tests/primitive_cases.py runs unchanged on either:
    h = P.dev(array)          a device copy of a numpy array (an output array goes up too: what the probe does not write stays)
    P.call("probe_x", h, 3)   launch; a non-zero launcher code raises at once, the device is synchronised once per launch
    P.get(h)                  the buffer's content as a numpy array of the original dtype and shape
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC_DIR = os.path.join(HERE, "devprobe")
SO = os.path.join(SRC_DIR, "libcc_devprobe.so")


def _sources():
    csrc = os.path.join(HERE, "..", "contour-context_amd", "csrc")
    srcs = [os.path.join(SRC_DIR, f) for f in ("devprobe.hip", "probes.inc")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    srcs.append(os.path.join(HERE, "..", "include", "cont2_amd.h"))
    return srcs


def build():
    """Compile the device probe library when it is missing or older than a source or a csrc header."""
    if os.path.exists(SO) and all(os.path.getmtime(s) <= os.path.getmtime(SO) for s in _sources()):
        return SO
    import cc_amd
    flags = cc_amd.load().HIPCC_FLAGS
    subprocess.check_call(["hipcc"] + flags + [os.path.join(SRC_DIR, "devprobe.hip"), "-o", SO])
    return SO


def _as_arg(v):
    if isinstance(v, (int, np.integer)):
        return C.c_long(int(v))
    raise TypeError("probe argument %r" % (v,))


class _Buf:
    def __init__(self, ptr, keep, dtype, shape):
        self.ptr, self.keep, self.dtype, self.shape = ptr, keep, dtype, shape


class EmuProbe:
    """The probe entry points of the CPU harness; "device" memory is numpy memory."""
    name = "harness"

    def __init__(self):
        import emu_api
        self.lib = C.CDLL(emu_api.build())

    def dev(self, arr, offset=0):
        a = np.array(arr, copy=True, order="C")
        return _Buf(a.ctypes.data + offset, a, a.dtype, a.shape)

    def get(self, h):
        return h.keep

    def call(self, fn, *args):
        f = getattr(self.lib, fn)
        f.restype = C.c_int
        rc = f(*[C.c_void_p(a.ptr) if isinstance(a, _Buf) else _as_arg(a) for a in args])
        if rc != 0:
            raise RuntimeError("%s: launcher returned %d" % (fn, rc))


class GpuProbe:
    """tests/devprobe/libcc_devprobe.so on the current HIP device; memory comes from torch."""
    name = "MI355X"

    def __init__(self):
        import torch
        self.torch = torch
        so = os.environ.get("CC_DEVPROBE_LIB")  # another build of the same library (mutation experiments on a scratch copy)
        if not so:
            try:
                so = build()
            except Exception as e:  # a missing probe library is an error, not a reason to skip
                raise RuntimeError("the device probe library is not built and cannot be built here: %s" % e)
        self.lib = C.CDLL(so)

    def dev(self, arr, offset=0):
        a = np.ascontiguousarray(arr)
        t = self.torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).cuda()
        return _Buf(t.data_ptr() + offset, t, a.dtype, a.shape)

    def get(self, h):
        return h.keep.cpu().numpy().view(h.dtype).reshape(h.shape)

    def call(self, fn, *args):
        f = getattr(self.lib, fn)
        f.restype = C.c_int
        rc = f(*[C.c_void_p(a.ptr) if isinstance(a, _Buf) else _as_arg(a) for a in args])
        if rc != 0:
            raise RuntimeError("%s: launcher returned HIP error %d" % (fn, rc))
        self.torch.cuda.synchronize()
