"""What the host test files of the ctypes front ends share (tests/test_{mesh_eval,tnt_eval,mesh_cull,tsdf,delaunay,
delaunay_predicates}_host.py): the emulated library, "run this test file as a child process over it" (an emulator abort fails one
test, not the session) and the host stand-ins for a product module's device seams.  Importing it puts tests/ and the package on
sys.path (a child process has no conftest)."""
import contextlib
import os
import re
import subprocess
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(TESTS)
PKG = os.path.join(ROOT, "gaussian-opacity-fields_amd")
for _p in (TESTS, PKG, os.path.join(TESTS, "hipemu")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GUARD = 256


def emulated_library():
    """-> the path of the emulated library, built where it is stale; skips the calling test where there is no host compiler"""
    import pytest
    import build_emu
    if not os.path.exists(build_emu.CXX):
        pytest.skip("no host clang++ (%s) to build the emulated library" % build_emu.CXX)
    return build_emu.build()


def run_child(test_file, case, tmp_path, *more, timeout, order=None, env=None, tag=""):
    """`python test_file case out.npz more...` with GOF_HIP_LIB naming the emulated library, under HIPEMU_ORDER=order and the extra
    environment `env` -> what the child saved, as a dictionary.  tag: tells the output files of one test apart where `env` does."""
    lib = emulated_library()
    name = "_".join([case, order or "forward"] + [str(m) for m in more] + ([tag] if tag else []))
    out = str(tmp_path / (re.sub(r"[^A-Za-z0-9.]+", "_", name) + ".npz"))
    env = dict(os.environ, GOF_HIP_LIB=lib, **(env or {}))
    if order:
        env["HIPEMU_ORDER"] = order
    r = subprocess.run([sys.executable, os.path.abspath(test_file), case, out] + [str(m) for m in more], env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, "emulated run of %s (order %s) failed (rc %d):\n%s\n%s" % (case, order, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return dict(np.load(out))


def install_seams(*modules, buffers="workspaces"):
    """The product modules run unchanged except for their device seams (the private names they bind from gof_native): the device
    check, the stream, the device context and the current device become host stand-ins, and a module's `torch` one whose empty()
    fills a buffer with 0xA5 and puts GUARD bytes behind it.  buffers: "workspaces" guards what is asked for as torch.empty(n,
    dtype=torch.uint8) and nothing else (mesh_eval, tnt_eval, delaunay); "all" guards and poisons every buffer (mesh_cull: the pad bits
    of its outputs must have been written as well); None leaves the module's torch alone (tsdf_fusion allocates through a seam of its
    own, by role).  -> check(): asserts that every guard is intact and returns the number of buffers handed out."""
    import torch
    held = []

    class TorchWithGuards:
        def __getattr__(self, k):
            return getattr(torch, k)

        @staticmethod
        def empty(*a, **k):
            k.pop("device", None)
            if buffers == "workspaces" and not (k.get("dtype") is torch.uint8 and len(a) == 1 and isinstance(a[0], int)):
                return torch.empty(*a, **k)
            shape = tuple(int(s) for s in (a if isinstance(a[0], int) else a[0]))
            nbytes = int(np.prod(shape)) * torch.empty(0, dtype=k["dtype"]).element_size()
            buf = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8)
            held.append((buf, nbytes))
            return buf[:nbytes].view(k["dtype"]).reshape(shape)

    def check():
        for buf, n in held:
            assert (buf[n:] == 0xA5).all(), "guard bytes behind a %d-byte buffer were overwritten" % n
        return len(held)
    for mod in modules:
        if buffers is not None:
            mod.torch = TorchWithGuards()
        mod._on_device = lambda t: True
        mod._stream = lambda: None
        mod._device_of = lambda t: contextlib.nullcontext()
        mod._device = lambda: torch.device("cpu")
    return check


def host_buffers(mod):
    """-> (alloc, down) of a child process: alloc(nbytes) is one more of the module's own poisoned, guarded buffers, down(t) a numpy copy"""
    import torch
    return (lambda nbytes: mod.torch.empty(int(nbytes), dtype=torch.uint8)), (lambda t: t.detach().numpy().copy())


def install_transfer_seams(*modules):
    """install_seams with every buffer guarded, and host stand-ins for the seams of the modules that move data between the host and
    the device (image_writer, png_reader, scene_images), each where a module has it: the device is "there", an upload, a download and a
    move to the device are copies, and a pinned buffer is one more poisoned, guarded buffer of the module's.  -> check()"""
    import torch
    check = install_seams(*modules, buffers="all")
    for mod in modules:
        stand_ins = {"_have_device": lambda: True, "_to_device": lambda t, dev: t.clone(), "_upload": lambda host, dev: host.clone(),
                     "_download": lambda t: t.clone(), "_pinned": lambda n, mod=mod: mod.torch.empty(int(n), dtype=torch.uint8)}
        for name, f in stand_ins.items():
            if hasattr(mod, name):
                setattr(mod, name, f)
    return check
