"""Generates tests/golden/ref_densify_golden.npz by EXECUTING the reference's own scene.gaussian_model.GaussianModel where it lies
(/root/reference; build container only -- the tests read the committed .npz): GaussianModel.densify_and_prune with everything it calls
(densify_and_clone, densify_and_split, densification_postfix, prune_points and the optimizer surgery), on CPU tensors.

  * `device="cuda"` / `.cuda()` are redirected to the CPU as make_golden.py / make_golden_train.py do.
  * torch.normal(mean, std) is replaced by mean + std * z with z taken in order from a recorded array (a CPU generator and a GPU
    generator do not produce the same stream); the z that were consumed and the shapes they were asked for, in order, are recorded.
  * every model is built as tests/devtools/dev_densify_check.py builds its models: the six parameters, training_setup, one Adam step
    so that moments exist, then the statistics.  What differs, and why:
      - the gradients of that step are +-2^-e (and zero for the SH bands 1..13 of f_rest) and f_rest holds multiples of 2^-7: the
        moments and f_rest stay identifiable per row and column, and the fixture compresses below the size limit;
      - `_scaling` is set AFTER the step to values s for which exp(s), exp(s) / 1.6 and log(exp(s) / 1.6) are all within 0.05 ulp of
        a float32 (and x / 1.6f == x * (1 / 1.6f)): a CPU and a GPU that each round these functions within an ulp still agree on
        every bit of the split Gaussians' new scaling, so the fixture can be held bit for bit on either.
  * the reference's sampled positions are compared here with a float64 evaluation of R(q) (std * z) + x from the same float32 inputs;
    the worst deviation in ulp of |x| + sum_j |R_ij| |std_j z_j| is recorded per case (`xyz_worst_ulp`) and asserted <= 8 at the
    end of this script (the tests would allow twice a recorded figure above 8, but only after that assertion is removed on purpose).
No reference code is copied.  The archive is written with fixed time stamps: running this twice gives the same bytes."""
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch
from torch import nn

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))
import densify_restatement as DR                                       # noqa: E402  (float64 positions, categories)

# ---- the reference hard-codes the device: redirect to the CPU ----
torch.Tensor.cuda = lambda self, *a, **k: self
nn.Module.cuda = lambda self, *a, **k: self


def _cpu(fn):
    def wrapped(*a, **k):
        k.pop("device", None)
        return fn(*a, **k)
    return wrapped


for _name in ("zeros", "ones", "empty", "full", "arange", "tensor"):
    setattr(torch, _name, _cpu(getattr(torch, _name)))
for _name in ("plyfile", "trimesh", "simple_knn", "simple_knn._C", "open3d", "cv2"):
    if _name not in sys.modules:
        sys.modules[_name] = types.ModuleType(_name)
sys.modules["plyfile"].PlyData = object
sys.modules["plyfile"].PlyElement = object
sys.modules["simple_knn._C"].distCUDA2 = lambda *a, **k: None
from scene.gaussian_model import GaussianModel                         # noqa: E402  (the reference's class)

F32 = np.float32
Z = {"all": None, "pos": 0, "shapes": []}


def _recorded_normal(mean, std):
    n = int(mean.shape[0])
    z = torch.from_numpy(Z["all"][Z["pos"]:Z["pos"] + n])
    assert z.shape[0] == n
    Z["pos"] += n
    Z["shapes"].append(tuple(int(s) for s in mean.shape))
    return mean + std * z


torch.normal = _recorded_normal


# ---- scalings whose exp / division / log round the same way on every device ----
def _near_float32(x64, tol=0.05):
    x32 = x64.astype(F32)
    return np.abs(x64 - x32.astype(np.float64)) <= tol * np.spacing(np.abs(x32)).astype(np.float64)


def robust_scalings(cand):
    cand = cand.astype(F32)
    e = np.exp(cand.astype(np.float64))
    sc = e.astype(F32)
    d = sc / F32(1.6)
    ln = np.log(d.astype(np.float64))
    ok = _near_float32(e) & (d == sc * (F32(1) / F32(1.6))) & _near_float32(ln)
    return cand[ok]


_prng = np.random.default_rng(20240611)
POOL = robust_scalings(np.log(np.exp(0.7 * _prng.standard_normal(3_000_000)) * 0.02))       # scales around 0.02, as dev_densify_check
POOL_BIG = robust_scalings(_prng.uniform(0.05, 1.2, 1_000_000))                              # scales in (1.05, 3.3)


def pick(rng, n, lo=None, hi=None, pool=None):
    pool = POOL if pool is None else pool
    if lo is not None:
        pool = pool[(np.exp(pool) > lo) & (np.exp(pool) < hi)]
    return pool[rng.integers(0, pool.shape[0], n)]


ARGS = dict(position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01, position_lr_max_steps=30000, feature_lr=0.0025,
            opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001, appearance_embeddings_lr=0.001, appearance_network_lr=0.001)
NAMES = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"), ("scaling", "_scaling"), ("rotation", "_rotation"))


def make_model(P, seed, percent_dense=0.01):
    rng = np.random.default_rng(seed)
    r = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(F32))          # noqa: E731
    pow2 = lambda *s: torch.from_numpy((rng.choice([-1.0, 1.0], s) * 2.0 ** -rng.integers(0, 16, s)).astype(F32))   # noqa: E731
    m = GaussianModel(3)
    m._xyz = nn.Parameter(r(P, 3))
    m._features_dc = nn.Parameter(r(P, 1, 3))
    m._features_rest = nn.Parameter(torch.round(0.1 * r(P, 15, 3) * 128) / 128)
    m._scaling = nn.Parameter(torch.from_numpy(pick(rng, P * 3).reshape(P, 3)))
    m._rotation = nn.Parameter(r(P, 4))
    m._opacity = nn.Parameter(2.5 * r(P, 1))
    m.max_radii2D = torch.zeros(P)
    m.filter_3D = torch.full((P, 1), 0.001)
    m.spatial_lr_scale = 1.0
    m.training_setup(types.SimpleNamespace(percent_dense=percent_dense, **ARGS))
    for grp in m.optimizer.param_groups:                       # one step so that every per-Gaussian tensor has Adam moments
        for p in grp["params"]:
            if p.shape[0] == P and grp["name"] in dict(NAMES):
                p.grad = pow2(*p.shape)
                if grp["name"] == "f_rest":
                    p.grad[:, 1:14] = 0.0
    m.optimizer.step()
    m.optimizer.zero_grad(set_to_none=True)
    with torch.no_grad():
        m._scaling.copy_(torch.from_numpy(pick(rng, P * 3).reshape(P, 3)))
    m.xyz_gradient_accum = torch.from_numpy(rng.random((P, 1), dtype=F32) * F32(0.002))
    m.xyz_gradient_accum_abs = torch.from_numpy(rng.random((P, 1), dtype=F32) * F32(0.004))
    m.xyz_gradient_accum_abs_max = torch.from_numpy(rng.random((P, 1), dtype=F32))
    m.denom = torch.from_numpy(rng.integers(0, 4, (P, 1)).astype(F32))            # zeros included: x / 0 = inf
    m.max_radii2D = torch.from_numpy(rng.random(P, dtype=F32) * F32(40))
    return m, rng


def set_rows(m, rows, accum=None, accum_abs=None, denom=None, scaling=None, opacity=None):
    with torch.no_grad():
        for t, v in ((m.xyz_gradient_accum, accum), (m.xyz_gradient_accum_abs, accum_abs), (m.denom, denom), (m._opacity, opacity)):
            if v is not None:
                t[rows, 0] = torch.as_tensor(np.asarray(v, dtype=F32))
        if scaling is not None:
            m._scaling[rows] = torch.as_tensor(np.asarray(scaling, dtype=F32))


def state_of(m):
    st = {"percent_dense": np.float64(m.percent_dense)}
    groups = {g["name"]: g for g in m.optimizer.param_groups}
    for name, attr in NAMES:
        p = getattr(m, attr)
        assert groups[name]["params"][0] is p
        st[name] = p.detach().numpy().copy()
        s = m.optimizer.state[p]
        st["m_" + name], st["v_" + name] = s["exp_avg"].numpy().copy(), s["exp_avg_sq"].numpy().copy()
    for name in DR.STATS + ("max_radii2D",):
        st[name] = getattr(m, name).numpy().copy()
    return st


out = {}
cases = []


def record(case, m, max_grad, min_opacity, extent, max_screen_size):
    before = state_of(m)
    zrng = np.random.default_rng(sum(case.encode()))
    Z["all"], Z["pos"], Z["shapes"] = zrng.standard_normal((6 * before["xyz"].shape[0] + 8, 3)).astype(F32), 0, []
    with torch.no_grad():
        ret = GaussianModel.densify_and_prune(m, max_grad, min_opacity, extent, max_screen_size)
    after = state_of(m)
    z = Z["all"][:Z["pos"]]
    # float64 evaluation of the sampled positions (decisions and everything else as in float32) and the reference's distance from it
    truth, ret64, shapes64, info = DR.densify_and_prune(before, max_grad, min_opacity, extent, max_screen_size, z, pos_dtype=np.float64)
    assert truth["xyz"].shape == after["xyz"].shape, (case, truth["xyz"].shape, after["xyz"].shape)
    s = info["sampled"]
    worst = 0.0
    if s.any():
        worst = float((np.abs(after["xyz"][s].astype(np.float64) - truth["xyz"][s]) / (2.0 ** -23 * info["mag"][s])).max())
    assert np.array_equal(after["xyz"][~s], truth["xyz"][~s].astype(F32))
    for k, v in before.items():
        out["%s.b.%s" % (case, k)] = v
    for k, v in after.items():
        if k != "percent_dense":
            out["%s.a.%s" % (case, k)] = v
    out[case + ".args"] = np.array([max_grad, min_opacity, extent, np.nan if max_screen_size is None else max_screen_size], dtype=np.float64)
    out[case + ".ret"] = np.array([int(x) for x in ret], dtype=np.int64)
    out[case + ".z"] = z
    out[case + ".draw_shapes"] = np.array(Z["shapes"], dtype=np.int64).reshape(-1, 2)
    out[case + ".xyz_f64"] = truth["xyz"]
    out[case + ".xyz_worst_ulp"] = np.float64(worst)
    cases.append(case)
    print("%-14s P %4d -> %4d  ret %s  draws %s  roles %s  worst position error %.2f ulp" % (
        case, before["xyz"].shape[0], after["xyz"].shape[0], tuple(int(x) for x in ret), Z["shapes"], np.bincount(info["role"], minlength=3).tolist(), worst))
    return before, after, info


MG, MO, EXT = 0.0002, 0.05, 3.0

# ---- P = 1: cloned, split, pruned to nothing ----
for case, big, opac in (("p1_clone", False, 2.0), ("p1_split", True, 2.0), ("p1_pruned", False, -5.0)):
    m, rng = make_model(1, 11)
    set_rows(m, [0], accum=[0.01], accum_abs=[0.01], denom=[2.0], opacity=[opac],
             scaling=[pick(rng, 3, 0.04, 0.2) if big else pick(rng, 3, 0.004, 0.025)])
    b, a, info = record(case, m, MG, MO, EXT, None)
    assert a["xyz"].shape[0] == (0 if case == "p1_pruned" else 2) and info["role"][0] == (2 if big else 1)

# ---- P = 2: one cloned, one split ----
m, rng = make_model(2, 12)
set_rows(m, [0, 1], accum=[0.01, 0.02], accum_abs=[0.01, 0.02], denom=[1.0, 3.0], opacity=[1.0, 3.0],
         scaling=[pick(rng, 3, 0.004, 0.025), pick(rng, 3, 0.04, 0.2)])
b, a, info = record("p2", m, MG, MO, EXT, None)
assert info["role"].tolist() == [1, 2] and a["xyz"].shape[0] == 4

# ---- P = 257, no screen-size limit; P = 600 with one, and with a negative one (every row pruned) ----
m, rng = make_model(257, 13)
b, a, info = record("p257", m, MG, MO, EXT, None)
assert min(np.bincount(info["role"], minlength=3)) > 0 and out["p257.ret"][2] > 0
m, rng = make_model(600, 14)
b, a, info = record("p600_ms20", m, MG, MO, EXT, 20)
assert min(np.bincount(info["role"], minlength=3)) > 0 and out["p600_ms20.ret"][2] > 0
m, rng = make_model(600, 14)
b, a, info = record("p600_msneg", m, MG, MO, EXT, -1)
assert a["xyz"].shape[0] == 0

# ---- P = 300, no |grads| >= max_grad: ratio = 0, Q = max(grads_abs), exactly the maximal rows are selected (a tie by construction) ----
m, rng = make_model(300, 15)
P = 300
with torch.no_grad():
    m.denom.copy_(torch.from_numpy(rng.integers(1, 4, (P, 1)).astype(F32)))
    m.xyz_gradient_accum.mul_(0.05)                                       # < 0.0001 / denom: below max_grad everywhere
top = [3, 77, 150, 151, 299]
set_rows(m, top, accum_abs=[0.5, 1.0, 2.0, 0.5, 1.0], denom=[1.0, 2.0, 4.0, 1.0, 2.0],
         scaling=[pick(rng, 3, 0.004, 0.025), pick(rng, 3, 0.04, 0.2), pick(rng, 3, 0.004, 0.025), pick(rng, 3, 0.04, 0.2), pick(rng, 3, 0.04, 0.2)])
b, a, info = record("p300_nonorm", m, MG, MO, EXT, None)
assert float(info["Q"]) == 0.5 and sorted(info["clone_idx"].tolist() + info["split_idx"].tolist()) == top

# ---- P = 300, constructed ties: small integers and powers of two, every quotient exact ----
# max_grad = 2^-12.  The size threshold is a float32 T1 = exp(s1) whose successor T2 = exp(s2), both to within 0.05 ulp, s2 with a
# well-rounded log(T2 / 1.6) as well: percent_dense = T1 (as a double), extent = 1
def threshold_pair():
    for s2 in POOL_BIG[(POOL_BIG >= 0.25) & (POOL_BIG < 0.5)]:
        T2 = F32(np.exp(np.float64(s2)))
        T1 = np.nextafter(T2, F32(0))
        for k in range(1, 6):
            s1 = F32(s2 - k * np.spacing(s2))
            if abs(np.exp(np.float64(s1)) - np.float64(T1)) <= 0.05 * np.spacing(T1):
                return s1, s2, T1, T2


S1, S2, T1, T2 = threshold_pair()
assert torch.exp(torch.tensor([S1, S2])).numpy().tolist() == [T1, T2] and T1 < T2 == np.nextafter(T1, F32(9))
m, rng = make_model(300, 16, percent_dense=float(T1))
MG_T, EXT_T = 2.0 ** -12, 1.0
den = rng.choice([1.0, 2.0, 4.0], P)
with torch.no_grad():
    m.denom[:, 0] = torch.from_numpy(den.astype(F32))
    m.xyz_gradient_accum[:, 0] = torch.from_numpy((rng.integers(0, 32, P) * 2.0 ** -16).astype(F32))      # quotient 16 * 2^-16 / 1 = max_grad: ties at random too
    m.xyz_gradient_accum_abs[:, 0] = torch.from_numpy((rng.integers(0, 64, P) * 2.0 ** -15).astype(F32))
small = lambda: pick(rng, 3, 0.004, 0.025)                               # noqa: E731
large = lambda: pick(rng, 3, 1.7, 3.3, pool=POOL_BIG)                      # noqa: E731
below = np.nextafter(F32(MG_T), F32(0))
at_th = lambda: np.array([S1, small()[0], small()[1]], dtype=F32)         # noqa: E731  exp(s1) = the threshold exactly
above_th = lambda: np.array([small()[0], S2, small()[1]], dtype=F32)      # noqa: E731  exp(s2) = one ulp above it
designed = {
    5: dict(accum=2.0 ** -11, denom=2.0, accum_abs=0.0, scaling=small()),      # quotient == max_grad, small -> cloned
    6: dict(accum=2.0 ** -11, denom=2.0, accum_abs=0.0, scaling=large()),      # quotient == max_grad, large -> split
    17: dict(accum=below, denom=1.0, accum_abs=0.0, scaling=small()),          # one ulp below max_grad -> stays
    18: dict(accum=below, denom=1.0, accum_abs=0.0, scaling=large()),
    40: dict(accum=2.0 ** -8, denom=1.0, accum_abs=0.0, scaling=at_th()),      # scale_max == threshold -> cloned (<=)
    41: dict(accum=2.0 ** -8, denom=1.0, accum_abs=0.0, scaling=above_th()),   # one ulp above -> split (>)
    90: dict(accum=0.0, denom=0.0, accum_abs=0.0, scaling=small()),            # 0 / 0 = NaN -> 0 -> stays
    91: dict(accum=0.0, denom=0.0, accum_abs=0.0, scaling=large()),
    120: dict(accum=2.0 ** -14, denom=0.0, accum_abs=2.0 ** -14, scaling=small()),   # x / 0 = inf -> cloned
    121: dict(accum=2.0 ** -14, denom=0.0, accum_abs=2.0 ** -14, scaling=large()),   # -> split
    200: dict(accum=-2.0 ** -10, denom=1.0, accum_abs=0.0, scaling=small()),   # negative, |g| = 4 max_grad, small -> cloned (magnitude)
    201: dict(accum=-2.0 ** -10, denom=1.0, accum_abs=0.0, scaling=large()),   # negative, large -> NOT split (raw value)
}
for row, v in designed.items():
    set_rows(m, [row], accum=[v["accum"]], accum_abs=[v["accum_abs"]], denom=[v["denom"]], scaling=[v["scaling"]], opacity=[2.0])
# a plateau of equal grads_abs around the quantile position: Q is that value whatever the last bit of the position
g = DR.quotient(m.xyz_gradient_accum.numpy(), m.denom.numpy())
ga = DR.quotient(m.xyz_gradient_accum_abs.numpy(), m.denom.numpy())
ratio = (np.abs(g) >= F32(MG_T)).astype(F32).mean(dtype=F32)
order = np.argsort(ga, kind="stable")
pos = int(round(float((F32(1) - ratio) * F32(P - 1))))
V = ga[order[pos]]
plateau = [int(i) for i in order[pos - 8:pos + 9] if int(i) not in designed]
assert len(plateau) >= 12 and np.isfinite(V) and V >= 1e-12
with torch.no_grad():
    for i in plateau:
        m.xyz_gradient_accum_abs[i, 0] = float(V) * float(m.denom[i, 0])
        m.xyz_gradient_accum[i, 0] = 0.0                                        # selected through grads_abs == Q alone
set_rows(m, plateau[:2], scaling=[small(), large()])
b, a, info = record("p300_ties", m, MG_T, MO, EXT_T, None)
assert float(info["Q"]) == float(V) and (DR.quotient(b["xyz_gradient_accum_abs"], b["denom"])[plateau] == V).all()
assert [int(info["role"][r]) for r in designed] == [1, 2, 0, 0, 1, 2, 0, 0, 1, 2, 1, 0], [int(info["role"][r]) for r in designed]
assert info["role"][plateau[0]] == 1 and info["role"][plateau[1]] == 2

worst = max(float(out[c + ".xyz_worst_ulp"]) for c in cases)
print("worst position error of the reference over all cases: %.2f ulp (bound 8)" % worst)
# The bound is checked HERE, on the CPU, before any GPU run.  Should the reference alone ever leave it: do not widen it -- the recorded
# `xyz_worst_ulp` is what the tests then double (densify_restatement.load_golden), and this assertion has to be taken out on purpose.
assert worst <= 8.0, "the reference's own sampled positions are %.2f ulp from their float64 evaluation: beyond the 8 ulp bound" % worst
out["cases"] = np.array(cases)

path = os.path.join(HERE, "ref_densify_golden.npz")
with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
    for k in sorted(out):
        buf = io.BytesIO()
        np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
        info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
        info.compress_type = zipfile.ZIP_DEFLATED
        info.external_attr = 0o644 << 16
        zf.writestr(info, buf.getvalue(), compresslevel=9)
print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")
