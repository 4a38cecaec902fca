"""Densification on the GPU (csrc/gaussian_model_ops.hip: gof_densify_select, gof_compact_rows, gof_rows_gather; train_epilogue/densify.py):

  B. the three kernels against the plain numpy restatement (tests/densify_restatement.py) -- exact equality throughout, these kernels
     compare, scan and move data -- at the sizes where a scan goes wrong (one element, the 256-thread block, the 1024-item tile, the
     switch of tile size and launch shape in device_scan_u32), with ties / NaN / inf / negative quotients, empty lists, misaligned
     pointers (the scalar path of rows_gather) and guard bands;
  C. train_epilogue.densify_and_prune against the results the REFERENCE's own method gave on CPU tensors
     (tests/golden/ref_densify_golden.npz), the recorded normal draws served in place of the generator;
  D. the rasterizer's learnt instance capacity over ten round trips between two models (diff_gaussian_rasterization/_backend._inherit_learnt).
Nothing here reads the reference or its staged copy."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch
from torch import nn

import densify_restatement as DR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32 = np.float32
# radix.hip: SCAN_DIRECT_MAX = 2048 workgroups, 256 threads, SCAN_ITEMS_SMALL = 4 items per thread: up to N* items device_scan_u32 runs
# tiles of 1024 items, above it tiles of 4096 (SCAN_ITEMS_BIG = 16)
N_STAR = 2048 * 256 * 4
SIZES = (1, 2, 255, 256, 257, 1023, 1024, 1025, 4097, N_STAR, N_STAR + 1)
_golden = {}


def golden():
    if not _golden:
        _golden.update(DR.load_golden(os.path.join(ROOT, "tests", "golden", "ref_densify_golden.npz")))
    return _golden


def D():
    import train_epilogue.densify as mod
    return mod


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- select -----------------------------------------------------------------------------------------------------------------
MAX_GRAD_T, Q_T, TH_T = 2.0 ** -12, 2.0 ** -9, 1.0
_below = np.nextafter(F32(MAX_GRAD_T), F32(0))
_th_up = np.nextafter(F32(TH_T), F32(2))
# one period of the tie pattern: (accum, denom, accum_abs, scale_max)
TIE_ROWS = (
    (2.0 ** -11, 2.0, 0.0, 0.5), (2.0 ** -11, 2.0, 0.0, 2.0),                # quotient == max_grad: cloned / split
    (_below, 1.0, 0.0, 0.5), (_below, 1.0, 0.0, 2.0),                        # one ulp below: stays
    (0.0, 1.0, Q_T, 0.5), (0.0, 4.0, 4 * Q_T, 2.0),                          # grads_abs == Q: cloned / split
    (0.0, 1.0, np.nextafter(F32(Q_T), F32(0)), 2.0),                         # one ulp below Q: stays
    (2.0 ** -8, 1.0, 0.0, TH_T), (2.0 ** -8, 1.0, 0.0, _th_up),              # scale_max == threshold: cloned; one ulp above: split
    (0.0, 0.0, 0.0, 0.5), (0.0, 0.0, 0.0, 2.0),                              # 0 / 0 = NaN -> 0: stays
    (2.0 ** -14, 0.0, 2.0 ** -14, 0.5), (2.0 ** -14, 0.0, 0.0, 2.0),         # x / 0 = inf: cloned / split
    (-2.0 ** -10, 1.0, 0.0, 0.5), (-2.0 ** -10, 1.0, 0.0, 2.0),              # negative past max_grad: cloned (magnitude) / NOT split (raw)
    (-2.0 ** -14, 0.0, 0.0, 0.5), (-2.0 ** -14, 0.0, 0.0, 2.0),              # -inf: cloned / not split
)
TIE_ROLES = (1, 2, 0, 0, 1, 2, 0, 1, 2, 0, 0, 1, 2, 1, 0, 1, 0)


def select_inputs(family, P, rng):
    """-> accum, accum_abs, denom, scale_max, max_grad, Q, size_threshold"""
    if family == "random":
        denom = rng.integers(0, 4, P).astype(F32)
        accum, accum_abs = rng.random(P, dtype=F32) * F32(0.002), rng.random(P, dtype=F32) * F32(0.004)
        smax = (np.exp(0.7 * rng.standard_normal(P)) * 0.02).astype(F32)
        ga = DR.quotient(accum_abs, denom)
        return accum, accum_abs, denom, smax, 0.0002, float(np.sort(ga)[int(0.7 * (P - 1))]), float(smax[P // 2])       # Q and the threshold are data values: ties
    if family == "ties":
        t = np.array(TIE_ROWS, dtype=F32)
        t = np.tile(t, (P // len(t) + 1, 1))[:P]
        return t[:, 0].copy(), t[:, 2].copy(), t[:, 1].copy(), t[:, 3].copy(), MAX_GRAD_T, Q_T, TH_T
    role = int(family[-1])                                                       # all0 / all1 / all2: two of the three lists are empty
    one = np.ones(P, dtype=F32)
    return (one * (0 if role == 0 else 1)), 0 * one, one, one * (2.0 if role == 2 else 0.5), 0.5, 3.0, 1.0


def run_select(args):
    accum, accum_abs, denom, smax, max_grad, Q, th = args
    got = D().select(dev(accum), dev(accum_abs), dev(denom), dev(smax), max_grad, torch.tensor([Q], dtype=torch.float32, device=DEV), th)
    want = DR.select(accum, accum_abs, denom, smax, max_grad, Q, th)
    for name, g, w in zip(("role", "keep_idx", "clone_idx", "split_idx"), got, want):
        g = host(g)
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s %s, expected %s %s" % (name, g.dtype, g.shape, w.dtype, w.shape)     # the counts
        assert np.array_equal(g, w), "%s differs first at %d" % (name, int(np.nonzero(g != w)[0][0]))
    return want


def test_the_tie_pattern_decides_as_the_rule_says():
    """the restatement on one period of the pattern, against roles written down by hand (>= / <=, NaN -> 0, +-inf, magnitude against raw)"""
    role = run_select(select_inputs("ties", len(TIE_ROWS), None))[0]
    assert role.tolist() == list(TIE_ROLES)


@pytest.mark.parametrize("P", SIZES)
def test_select_equals_the_restatement(P):
    """role, the three ascending lists and their counts: random statistics (x/0 = inf included; Q and the size threshold are values of
    the data), the tiled tie / NaN / inf / negative pattern, and the degenerate cases all-stay / all-cloned / all-split (two lists empty)"""
    rng = np.random.default_rng(P)
    for family in ("random", "ties", "all0", "all1", "all2"):
        role = run_select(select_inputs(family, P, rng))[0]
        if family.startswith("all"):
            assert (role == int(family[-1])).all()


def test_select_carries_the_scan_across_tiles_at_the_switch_of_tile_size():
    """N* + 1 rows with selected rows only at 0, N* - 1 and N*: the last entry of each list crosses every tile boundary's carry"""
    P = N_STAR + 1
    accum, denom, smax = np.zeros(P, dtype=F32), np.ones(P, dtype=F32), np.full(P, 0.5, dtype=F32)
    accum[[0, N_STAR - 1, N_STAR]] = 1.0
    smax[[0, N_STAR]] = 2.0
    role, keep, clone, split = run_select((accum, np.zeros(P, dtype=F32), denom, smax, 0.5, 3.0, 1.0))
    assert clone.tolist() == [N_STAR - 1] and split.tolist() == [0, N_STAR] and keep.shape[0] == P - 2 and keep[-1] == N_STAR - 1


# ---- compact_rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_compact_rows_equals_the_restatement(n):
    """with and without src_rows (negative ids included, as the method passes them); nothing kept, everything kept; keep bytes 2 and 255
    count as kept"""
    rng = np.random.default_rng(n + 7)
    src = rng.integers(-n, n, n).astype(np.int32)
    keeps = {"random": (rng.random(n) < 0.4).astype(np.uint8), "none": np.zeros(n, dtype=np.uint8), "all": np.ones(n, dtype=np.uint8),
             "bytes 2 and 255": rng.choice(np.array([0, 2, 255], dtype=np.uint8), n)}
    if n > N_STAR:
        only = np.zeros(n, dtype=np.uint8)
        only[[0, N_STAR - 1, N_STAR]] = 1
        keeps["first, N* - 1, N*"] = only
    for name, keep in keeps.items():
        for s in (None, src):
            got = host(D().compact_rows(dev(keep), None if s is None else dev(s)))
            want = DR.compact_rows(keep, s)
            assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (name, s is not None)
    got = host(D().compact_rows(dev(keeps["random"].astype(bool))))                 # the method hands in a bool tensor
    assert np.array_equal(got, DR.compact_rows(keeps["random"]))


# ---- rows_gather ------------------------------------------------------------------------------------------------------------
GUARD_BITS = 0x7FC0BEEF          # a NaN with a payload


def offset_tensor(a, offset):
    """the array on the device starting `offset` floats into a larger buffer: offset 0 is 16-byte aligned, 1 is not"""
    a = np.ascontiguousarray(a, dtype=F32)
    big = torch.empty(a.size + 8, dtype=torch.float32, device=DEV)
    assert big.data_ptr() % 16 == 0
    t = big[offset:offset + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == (4 * offset) % 16 and t.is_contiguous()
    return t


def gather_in_guard_band(rows, src_t, extra_t, per, out_offset=0, guard=64):
    """gof_rows_gather on a slice of a buffer filled with a NaN pattern -> (result, band untouched)"""
    mod = D()
    n = int(rows.shape[0])
    buf = torch.full((2 * guard + n * per + 8,), GUARD_BITS, dtype=torch.int32, device=DEV)
    out = buf[guard + out_offset:guard + out_offset + n * per]
    rows_t = dev(rows.astype(np.int32)) if n else torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = mod.lib.gof_rows_gather(n, per, rows_t.data_ptr(), src_t.data_ptr(), None if extra_t is None else extra_t.data_ptr(), out.data_ptr(), mod.B._stream())
    assert rc == 0, mod.lib.gof_last_error()
    torch.cuda.synchronize()
    b = host(buf)
    band = np.concatenate((b[:guard + out_offset], b[guard + out_offset + n * per:]))
    return b[guard + out_offset:guard + out_offset + n * per].view(F32).reshape(n, per), bool((band == GUARD_BITS).all())


@pytest.mark.parametrize("per", (1, 3, 4, 45, 48))
def test_rows_gather_equals_the_restatement(per):
    """repeated non-negative ids mixed with negative ids into `extra`; extra=None gives exact zeros; for 4 and 48 floats per row a source,
    an `extra` or an output one float off 16-byte alignment takes the scalar path; nothing is written outside the output"""
    rng = np.random.default_rng(per)
    S, E = 97, 31
    src, extra = rng.standard_normal((S, per)).astype(F32), rng.standard_normal((E, per)).astype(F32)
    variants = [(0, 0, 0)] + ([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)] if per % 4 == 0 else [(1, 1, 1)])
    for n in (1, 257, 1000):
        rows = rng.integers(-E, S, n).astype(np.int32)
        rows[0] = -E if n == 1 else rows[0]
        if n > 1:
            rows[:6] = (5, 5, -1, -E, S - 1, 0)
        for so, eo, oo in variants:
            src_t, extra_t = offset_tensor(src, so), offset_tensor(extra, eo)
            got, band_ok = gather_in_guard_band(rows, src_t, extra_t, per, oo)
            assert band_ok and np.array_equal(bits(got), bits(DR.rows_gather(rows, src, extra))), (n, so, eo, oo)
            got, band_ok = gather_in_guard_band(rows, src_t, None, per, oo)
            want = DR.rows_gather(rows, src, None)
            assert band_ok and np.array_equal(bits(got), bits(want)) and (bits(got[rows < 0]) == 0).all(), (n, so, eo, oo, "extra=None")
        got = host(D().rows_gather(dev(rows), offset_tensor(src, 1), offset_tensor(extra, 0)))      # the Python mirror
        assert np.array_equal(bits(got), bits(DR.rows_gather(rows, src, extra)))
    got, band_ok = gather_in_guard_band(np.zeros(0, dtype=np.int32), offset_tensor(src, 0), None, per)       # n_rows == 0
    assert band_ok and got.shape == (0, per)
    assert D().rows_gather(dev(np.zeros(0, dtype=np.int32)), dev(src), None).shape == (0, per)


def test_rows_gather_keeps_trailing_dimensions():
    rng = np.random.default_rng(3)
    src, extra = rng.standard_normal((40, 15, 3)).astype(F32), rng.standard_normal((9, 15, 3)).astype(F32)
    rows = rng.integers(-9, 40, 300).astype(np.int32)
    got = host(D().rows_gather(dev(rows), dev(src), dev(extra)))
    assert got.shape == (300, 15, 3) and np.array_equal(bits(got), bits(DR.rows_gather(rows, src, extra)))


# ---- argument errors --------------------------------------------------------------------------------------------------------
def test_densify_argument_errors():
    """a negative size, a workspace one byte short and a NULL list pointer are refused with gof_last_error set and nothing launched
    (every output still holds its sentinel afterwards)"""
    mod = D()
    lib, stream = mod.lib, mod.B._stream
    P = 300
    f = lambda v: torch.full((P,), v, dtype=torch.float32, device=DEV)                      # noqa: E731
    accum, accum_abs, denom, smax, q = f(1.0), f(1.0), f(1.0), f(0.5), torch.ones(1, device=DEV)
    role = torch.full((P,), 77, dtype=torch.uint8, device=DEV)
    lists = [torch.full((P,), -7, dtype=torch.int32, device=DEV) for _ in range(4)]
    nb = lib.gof_densify_ws_bytes(P)
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    keep = torch.ones(P, dtype=torch.uint8, device=DEV)
    counts = (C.c_int64 * 3)(5, 5, 5)
    cnt = C.c_int64(5)
    rows = torch.zeros(P, dtype=torch.int32, device=DEV)
    src = torch.ones((P, 4), device=DEV)
    out = torch.full((P, 4), -7.0, device=DEV)

    def select(n=P, keep_ptr=lists[0].data_ptr(), ws_bytes=nb):
        return lib.gof_densify_select(n, accum.data_ptr(), accum_abs.data_ptr(), denom.data_ptr(), smax.data_ptr(), 0.5, q.data_ptr(), 1.0, role.data_ptr(),
                                      keep_ptr, lists[1].data_ptr(), lists[2].data_ptr(), ws.data_ptr(), ws_bytes, counts, stream())

    def compact(n=P, out_ptr=lists[3].data_ptr(), ws_bytes=nb):
        return lib.gof_compact_rows(n, keep.data_ptr(), None, out_ptr, ws.data_ptr(), ws_bytes, C.byref(cnt), stream())

    def gather(n=P, per=4, rows_ptr=rows.data_ptr()):
        return lib.gof_rows_gather(n, per, rows_ptr, src.data_ptr(), None, out.data_ptr(), stream())

    for call, word in ((lambda: select(n=-1), "points"), (lambda: select(ws_bytes=nb - 1), "workspace"), (lambda: select(keep_ptr=None), "NULL"),
                       (lambda: compact(n=-1), "row count"), (lambda: compact(ws_bytes=nb - 1), "workspace"), (lambda: compact(out_ptr=None), "NULL"),
                       (lambda: gather(n=-1), "sizes"), (lambda: gather(per=0), "sizes"), (lambda: gather(rows_ptr=None), "NULL")):
        rc = call()
        msg = lib.gof_last_error().decode(errors="replace")
        assert rc != 0 and word in msg, (rc, msg, word)
    torch.cuda.synchronize()
    assert (role == 77).all() and all((l == -7).all() for l in lists) and (out == -7.0).all() and (ws == 0).all()
    assert select() == 0 and compact() == 0 and gather() == 0                             # the same calls, unbroken, go through
    torch.cuda.synchronize()
    assert list(counts) == [P, P, 0] and cnt.value == P and (role == 1).all() and (out == 1.0).all()


# ---- C. the method against the reference's recorded results ------------------------------------------------------------------------
def build_rotation(r):
    """rotation matrices of (n, 4) quaternions (w, x, y, z), normalised first: the standard unit-quaternion formula"""
    q = r / torch.sqrt((r * r).sum(dim=1))[:, None]
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.zeros((q.size(0), 3, 3), device=r.device)
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    return R


ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}


ACTIVATIONS = {
    # what GaussianModel.setup_functions installs: the device's float32 routines
    "float32": (torch.exp, torch.log, torch.sigmoid),
    # the same functions evaluated in float64 and rounded once: correctly rounded on any device
    "float64": (lambda x: torch.exp(x.double()).float(), lambda x: torch.log(x.double()).float(), lambda x: torch.sigmoid(x.double()).float()),
}


class Model:
    """what train_epilogue.densify_and_prune touches of a GaussianModel: the attributes, the activations, the optimizer.
    activations="float32": torch.exp / torch.log / torch.sigmoid as the real model hands them over.  The device's float32 exp and log
    are allowed an ulp and use it: on the MI355X the new scaling log(exp(s) / 1.6) of case p2's split Gaussian came out one ulp from
    the CPU's in two of three components (bits 3227568371 / 3228001781 against 3227568370 / 3228001780), nothing else differed.
    activations="float64": the same functions correctly rounded.  The fixture's scalings are chosen so that the correctly rounded
    values are what the reference's CPU run gave, so with these the recorded result can be held bit for bit on any device."""

    def __init__(self, before, fused_adam, extra_groups=(), extra_states=None, activations="float64"):
        import train_epilogue as T
        self.scaling_activation, self.scaling_inverse_activation, self.opacity_activation = ACTIVATIONS[activations]
        self.percent_dense = float(before["percent_dense"])
        groups = []
        for name in DR.PARAMS:
            setattr(self, ATTR[name], nn.Parameter(dev(before[name]).requires_grad_(True)))
            groups.append({"params": [getattr(self, ATTR[name])], "lr": 0.001, "name": name})
        groups += [{"params": [p], "lr": 0.001, "name": n} for n, p in extra_groups]
        self.optimizer = (T.FusedAdam if fused_adam else torch.optim.Adam)(groups, lr=0.0, eps=1e-15)
        for name in DR.PARAMS:                                                     # the recorded moments of the one Adam step
            self.optimizer.state[getattr(self, ATTR[name])] = {"step": torch.tensor(1.0), "exp_avg": dev(before["m_" + name]), "exp_avg_sq": dev(before["v_" + name])}
        for n, p in extra_groups:
            self.optimizer.state[p] = extra_states[n]
        for name in DR.STATS + ("max_radii2D",):
            setattr(self, name, dev(before[name]))

    get_scaling = property(lambda self: self.scaling_activation(self._scaling))
    get_xyz = property(lambda self: self._xyz)


def run_method(case, fused_adam, monkeypatch, extra_groups=(), extra_states=None, activations="float64"):
    """-> the model after train_epilogue.densify_and_prune, the return triple, the shapes torch.normal was asked for, the old parameters"""
    import train_epilogue as T
    c = golden()[case]
    utils = types.ModuleType("utils")
    utils.__path__ = []
    general = types.ModuleType("utils.general_utils")
    general.build_rotation = build_rotation
    utils.general_utils = general
    monkeypatch.setitem(sys.modules, "utils", utils)
    monkeypatch.setitem(sys.modules, "utils.general_utils", general)
    z, asked, taken = dev(c["z"]), [], [0]

    def recorded_normal(mean, std):
        n = int(mean.shape[0])
        asked.append(tuple(int(s) for s in mean.shape))
        assert tuple(std.shape) == tuple(mean.shape) and taken[0] + n <= z.shape[0]
        out = mean + std * z[taken[0]:taken[0] + n]
        taken[0] += n
        return out
    monkeypatch.setattr(torch, "normal", recorded_normal)
    m = Model(c["before"], fused_adam, extra_groups, extra_states, activations)
    old = [getattr(m, a) for a in ATTR.values()]
    ret = T.densify_and_prune(m, c["max_grad"], c["min_opacity"], c["extent"], c["max_screen_size"])
    torch.cuda.synchronize()
    assert taken[0] == z.shape[0]
    return m, tuple(int(x) for x in ret), asked, old


CASES = ("p1_clone", "p1_split", "p1_pruned", "p2", "p257", "p600_ms20", "p600_msneg", "p300_nonorm", "p300_ties")
# With the device's float32 exp the tie case is left out: its "scale_max == threshold" row needs exp(s1) to be one particular float,
# which a routine that is allowed an ulp does not promise (a property of the routine, not of densify.py); every other decision of
# every other case has a margin of many ulp.
METHOD_RUNS = [(c, a) for a in ("float64", "float32") for c in CASES if not (a == "float32" and c == "p300_ties")]


@pytest.mark.parametrize("fused_adam", (False, True), ids=("torch_adam", "fused_adam"))
@pytest.mark.parametrize("case,activations", METHOD_RUNS, ids=["%s-%s" % r for r in METHOD_RUNS])
def test_densify_and_prune_equals_the_references_recorded_result(case, activations, fused_adam, monkeypatch):
    """Return triple and final P; the order and shapes of the normal draws (clones first, then splits: "same generator consumption");
    every parameter, both Adam moments of every group, the reset statistics and max_radii2D bit for bit -- except the sampled positions,
    held to 8 ulp of |x| + sum_j |R_ij| |std_j z_j| around their float64 evaluation, the bound the fixture's generator put on the
    reference's own CPU result (its worst case: 2.66 ulp); each new nn.Parameter is the one in the optimizer's group and the old ones
    are gone from optimizer.state.
    Run with correctly rounded activations (bit for bit throughout) and again with the device's float32 exp / log / sigmoid.  In the
    second run one more tensor has a tolerance, the NEW scaling log(exp(s) / 1.6) of a split's samples: exp within an ulp and the product
    with 1 / 1.6f move the argument by at most 2 x 2^-23 relative, which is 2 x 2^-23 absolute in the logarithm; log itself adds an
    ulp of the result, the recorded value's own rounding 0.55 ulp.  Everything else, copied scalings included, stays bit for bit."""
    c = golden()[case]
    m, ret, asked, old = run_method(case, fused_adam, monkeypatch, activations=activations)
    want = c["after"]
    assert ret == c["ret"] and int(m._xyz.shape[0]) == want["xyz"].shape[0]
    assert asked == c["draw_shapes"]
    _, _, _, info = DR.densify_and_prune(c["before"], c["max_grad"], c["min_opacity"], c["extent"], c["max_screen_size"], c["z"])
    s = info["sampled"]
    groups = {g["name"]: g for g in m.optimizer.param_groups}
    for name, attr in ATTR.items():
        p = getattr(m, attr)
        assert isinstance(p, nn.Parameter) and p.requires_grad and groups[name]["params"][0] is p and len(groups[name]["params"]) == 1
        got = host(p)
        assert got.shape == want[name].shape and got.dtype == want[name].dtype, name
        if name == "xyz":
            assert np.array_equal(bits(got[~s]), bits(want[name][~s]))
            err = np.abs(got[s].astype(np.float64) - c["xyz_f64"][s]) / (2.0 ** -23 * info["mag"][s])
            print("%s: sampled positions up to %.2f ulp from float64 (bound %.1f)" % (case, err.max() if err.size else 0.0, c["bound_ulp"]))
            assert (err <= c["bound_ulp"]).all(), "sampled positions up to %.2f ulp away (bound %.1f)" % (err.max(), c["bound_ulp"])
        elif name == "scaling" and activations == "float32":
            new = info["split_sample"]
            assert np.array_equal(bits(got[~new]), bits(want[name][~new]))
            tol = 2 * 2.0 ** -23 + 1.55 * np.spacing(np.abs(want[name][new])).astype(np.float64)
            err = np.abs(got[new].astype(np.float64) - want[name][new])
            print("%s: new scalings up to %.2f ulp from the recorded ones" % (case, (err / np.spacing(np.abs(want[name][new]))).max() if err.size else 0.0))
            assert (err <= tol).all(), "new scalings up to %.3g away" % err.max()
        else:
            assert np.array_equal(bits(got), bits(want[name])), name
        st = m.optimizer.state[p]
        for k, mom in (("exp_avg", "m_"), ("exp_avg_sq", "v_")):
            assert st[k].shape == p.shape and np.array_equal(bits(host(st[k])), bits(want[mom + name])), (name, k)
    assert not any(o in m.optimizer.state for o in old) and len(m.optimizer.state) == 6
    for name in DR.STATS + ("max_radii2D",):
        t = getattr(m, name)
        assert t.dtype == torch.float32 and np.array_equal(bits(host(t)), bits(want[name])) and host(t).shape == want[name].shape, name


def test_densify_and_prune_leaves_the_groups_that_are_not_per_gaussian_alone(monkeypatch):
    """SKIP_GROUPS: an optimizer that also holds `appearance_embeddings` / `appearance_network` groups keeps their tensors and state"""
    import train_epilogue.densify as mod
    assert set(mod.SKIP_GROUPS) == {"appearance_embeddings", "appearance_network"}
    emb = nn.Parameter(torch.randn(257, 8, device=DEV))           # as many rows as Gaussians: only the group's NAME protects it
    net = nn.Parameter(torch.randn(5, 3, device=DEV))
    extra = (("appearance_embeddings", emb), ("appearance_network", net))
    before = {n: (p.detach().clone(), torch.randn_like(p), torch.rand_like(p)) for n, p in extra}
    states = {n: {"step": torch.tensor(1.0), "exp_avg": before[n][1].clone(), "exp_avg_sq": before[n][2].clone()} for n, _ in extra}
    m, ret, asked, old = run_method("p257", False, monkeypatch, extra, states)
    assert ret == golden()["p257"]["ret"] and len(m.optimizer.state) == 8
    groups = {g["name"]: g for g in m.optimizer.param_groups}
    for n, p in extra:
        assert groups[n]["params"] == [p] and groups[n]["params"][0] is p and torch.equal(p.detach(), before[n][0])
        assert m.optimizer.state[p] is states[n]
        assert torch.equal(states[n]["exp_avg"], before[n][1]) and torch.equal(states[n]["exp_avg_sq"], before[n][2])


# ---- D. learnt capacity over round trips between two models ---------------------------------------------------------------------------
def test_learnt_capacity_stays_put_when_two_models_alternate():
    """scene_frustum of 3000 Gaussians at 64x64 and its first 2000, rendered alternately for ten round trips: every visit gives the first
    visit's bits, the learnt capacity after the last round trip is that after the second, and no fused frame is redone after the second.
    Forward only, so of the three inherited values only the instance capacity is exercised here; the mask and record needs (learnt at
    a backward) rest on the host tests of tests/test_host_api.py."""
    import synthetic_scenes as S
    from gpu_common import to_dev, settings_from
    from diff_gaussian_rasterization import GaussianRasterizer, _backend as B
    sc = S.scene_frustum(3000, W=64, H=64, focal=60.0, seed=21, kernel_size=0.1)
    sd = to_dev(sc, DEV)
    rast = GaussianRasterizer(settings_from(sd))
    per_gaussian = ("means3D", "shs", "opacities", "scales", "rotations")

    def render(n):
        a = {k: sd[k][:n].contiguous() for k in per_gaussian}
        with torch.no_grad():
            color, radii = rast(means3D=a["means3D"], means2D=torch.zeros_like(a["means3D"]), shs=a["shs"], opacities=a["opacities"],
                                scales=a["scales"], rotations=a["rotations"])
        return host(color), host(radii)
    keys = [("cuda:0", n, 64, 64) for n in (3000, 2000)]
    learnt = (B._capacity, B._mask_need, B._staged_need) + tuple(B._sized_for)
    saved = [{k: d.pop(k) for k in keys if k in d} for d in learnt]
    recent = B._recent_P.pop(("cuda:0", 64, 64), None)
    try:
        first, caps, redone = {}, [], []
        for trip in range(10):
            for n in (3000, 2000):
                color, radii = render(n)
                if n not in first:
                    first[n] = (color, radii)
                assert np.array_equal(bits(color), bits(first[n][0])) and np.array_equal(radii, first[n][1]), (trip, n)
            caps.append({k: v for k, v in B._capacity.items() if k[2:] == (64, 64)})
            redone.append(B._stats["fused_redone_frames"])
        assert len(caps[1]) == 1 and caps[9] == caps[1], (caps[1], caps[9])
        assert redone[9] == redone[1], redone
    finally:
        for d, s in zip(learnt, saved):
            for k in keys:
                d.pop(k, None)
            d.update(s)
        B._recent_P.pop(("cuda:0", 64, 64), None)
        if recent is not None:
            B._recent_P[("cuda:0", 64, 64)] = recent
