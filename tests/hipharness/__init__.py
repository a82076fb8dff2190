"""HIP harness of the deflate block pricing (TEST INFRASTRUCTURE; see dfl_trees.hip): built at test time with
hipcc --offload-arch=gfx950, from the product's own device header."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "snacc_amd", "csrc")
_SO = os.path.join(_HERE, "libdfl_trees.so")
_lib = None

HIST = 320          # DFL_HIST: literal/length counts at 0..285, distance counts at DOFF..DOFF + 29
DOFF = 288
WAVES = 4           # DFL_WAVES: one histogram per wave, four per workgroup
MAX_HISTS = 4 * 512


def build():
    srcs = [os.path.join(_HERE, "dfl_trees.hip"), os.path.join(_CSRC, "snk_deflate.hip.h")]
    if not os.path.exists(_SO) or any(os.path.getmtime(_SO) < os.path.getmtime(s) for s in srcs):
        hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
        subprocess.check_call([hipcc if os.path.exists(hipcc) else "hipcc", "-O3", "-std=c++17", "-fPIC", "-shared",
                               "-Wall", "-Wno-unused-function", "--offload-arch=gfx950", "-I", _CSRC,
                               "-o", _SO, os.path.join(_HERE, "dfl_trees.hip")])
    return _SO


def run(hists, mode=0):
    """hists: (n, 286 + 30) counts (literal/length, then distance).  mode 0: the choice dfl_flush_body makes;
    1: the LDS builder for all.  Returns (opt_len[n], static_len[n], lds_used[n])."""
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
        _lib.dfl_trees_run.restype = ctypes.c_int
        _lib.dfl_trees_run.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    h = np.asarray(hists)
    assert h.ndim == 2 and h.shape[1] == 316 and 0 < len(h) <= MAX_HISTS
    assert h.min() >= 0 and h.sum(axis=1).max() < 1 << 16     # the LDS builder keeps node counts in u16
    buf = np.zeros((len(h), HIST), dtype=np.uint32)
    buf[:, :286] = h[:, :286]
    buf[:, DOFF:DOFF + 30] = h[:, 286:]
    buf[:, 256] = 1                                            # END_BLOCK, as dfl_hist_reset and zlib have it
    out = np.zeros((len(h), 3), dtype=np.int64)
    rc = _lib.dfl_trees_run(buf.ctypes.data, len(h), mode, out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"dfl_trees_run: HIP error {rc}")
    return out[:, 0], out[:, 1], out[:, 2]
