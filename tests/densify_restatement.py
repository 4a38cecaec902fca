"""Plain numpy restatement of densification (GaussianModel.densify_and_prune and the three device primitives it is built on in
train_epilogue/densify.py), written from the RULE, one sequential step after the other, the way the reference's method proceeds:

  grads     = xyz_gradient_accum / denom, NaN -> 0 (float32 IEEE division: x/0 = +-inf stays); grads_abs likewise
  ratio     = mean(|grads| >= max_grad);  Q = quantile(grads_abs, 1 - ratio) (linear interpolation)
  clone     where (|grads| >= max_grad or |grads_abs| >= Q) and max(exp(scaling)) <= percent_dense * extent
  split     where ( grads  >= max_grad or  grads_abs  >= Q) and max(exp(scaling)) >  percent_dense * extent
  clones    are appended (one new Gaussian: a sample around the original, everything else copied, zero Adam moments)
  splits    are appended twice (samples, scaling log(exp(scaling) / 1.6), rest copied, zero moments) and the originals leave
  prune     sigmoid(opacity) < min_opacity; with a max_screen_size also 0 > max_screen_size (max_radii2D was zeroed when the new
            Gaussians were appended) and max(exp(scaling)) > 0.1 * extent
  the four statistics and max_radii2D end as zeros of the final length.

No torch, no device library: tests/test_densify_host.py holds it to the reference's recorded results (tests/golden/ref_densify_golden.npz),
tests/test_densify_gpu.py holds the kernels and the method to it."""
import numpy as np

F32 = np.float32
PARAMS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
STATS = ("xyz_gradient_accum", "xyz_gradient_accum_abs", "xyz_gradient_accum_abs_max", "denom")
N_SPLIT = 2


def quotient(accum, denom):
    """accum / denom in float32 with NaN (0/0) -> 0; +-inf (x/0) stays"""
    with np.errstate(all="ignore"):
        g = np.asarray(accum, dtype=F32).reshape(-1) / np.asarray(denom, dtype=F32).reshape(-1)
    g[np.isnan(g)] = F32(0)
    return g


def select(accum, accum_abs, denom, scale_max, max_grad, Q, size_threshold):
    """-> role (uint8: 0 stays, 1 cloned, 2 split), keep_idx (role != 2), clone_idx, split_idx; ascending int32"""
    g, ga = quotient(accum, denom), quotient(accum_abs, denom)
    mg, q, th = F32(max_grad), F32(Q), F32(size_threshold)
    with np.errstate(invalid="ignore"):
        sel_clone = (np.abs(g) >= mg) | (np.abs(ga) >= q)          # the norm over the size-1 last dimension is the magnitude
        sel_split = (g >= mg) | (ga >= q)                          # the raw values
        small = np.asarray(scale_max, dtype=F32).reshape(-1) <= th
    role = np.where(small, np.where(sel_clone, 1, 0), np.where(sel_split, 2, 0)).astype(np.uint8)
    idx = np.arange(role.shape[0], dtype=np.int32)
    return role, idx[role != 2], idx[role == 1], idx[role == 2]


def compact_rows(keep, src_rows=None):
    """the rows i (or src_rows[i]) whose keep byte is non-zero, in order (int32)"""
    keep = np.asarray(keep).reshape(-1)
    rows = np.arange(keep.shape[0], dtype=np.int32) if src_rows is None else np.asarray(src_rows, dtype=np.int32)
    return rows[keep != 0]


def rows_gather(rows, src, extra):
    """out[r] = src[rows[r]] if rows[r] >= 0 else extra[-rows[r] - 1] (zeros where extra is None)"""
    rows = np.asarray(rows, dtype=np.int64)
    out = np.zeros((rows.shape[0],) + tuple(src.shape[1:]), dtype=src.dtype)
    old = rows >= 0
    out[old] = src[rows[old]]
    if extra is not None:
        out[~old] = extra[-rows[~old] - 1]
    return out


def quantile(values, q):
    """linear-interpolation quantile of a 1-D float32 array at the float32 level q in [0, 1], in float32"""
    s = np.sort(np.asarray(values, dtype=F32))
    pos = F32(q) * F32(s.shape[0] - 1)
    lo = int(np.floor(pos))
    hi = min(lo + 1, s.shape[0] - 1)
    w = F32(pos - F32(lo))
    with np.errstate(all="ignore"):
        return F32(s[lo] + w * (s[hi] - s[lo])) if w < 0.5 else F32(s[hi] - (s[hi] - s[lo]) * (F32(1) - w))


def rotation_matrices(q, dtype=F32):
    """(n, 4) quaternions (w, x, y, z), normalised here -> (n, 3, 3)"""
    q = np.asarray(q, dtype=dtype)
    q = q / np.sqrt((q * q).sum(axis=1, dtype=dtype))[:, None]
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3), dtype=dtype)
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    return R


def sample_positions(xyz, scale, rotation, z, dtype=F32):
    """R(q) (scale * z) + xyz and the magnitude |xyz| + sum_j |R_ij| |scale_j z_j| its rounding error is measured against"""
    R = rotation_matrices(rotation, dtype)
    s = np.asarray(scale, dtype=dtype) * np.asarray(z, dtype=dtype)
    x = np.asarray(xyz, dtype=dtype)
    pos = (R * s[:, None, :]).sum(axis=2, dtype=dtype) + x
    mag = np.abs(x.astype(np.float64)) + (np.abs(R.astype(np.float64)) * np.abs(s.astype(np.float64))[:, None, :]).sum(axis=2)
    return pos, mag


def exp32(x):
    """exp / log of float32 values evaluated in float64 and rounded once (numpy's float32 routines are allowed more than an ulp)"""
    return np.exp(np.asarray(x, dtype=F32).astype(np.float64)).astype(F32)


def log32(x):
    return np.log(np.asarray(x, dtype=F32).astype(np.float64)).astype(F32)


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return (1.0 / (1.0 + np.exp(-np.asarray(x, dtype=F32).astype(np.float64)))).astype(F32)


def densify_and_prune(state, max_grad, min_opacity, extent, max_screen_size, draws, pos_dtype=F32):
    """state: the six parameters under PARAMS, their Adam moments under "m_<name>" / "v_<name>", the four STATS, "max_radii2D" and the
    scalar "percent_dense".  draws: (n, 3) standard-normal samples, used in order in place of the generator.
    -> (new state, (cloned, split, pruned), [shape of every draw asked for, in order], info) where info carries the index lists, Q, and
    for every final row the rounding magnitude of a sampled position (0 for rows that were not sampled), whether it was sampled, and
    whether it is one of a split's two samples (the rows whose scaling is newly computed).
    pos_dtype=float64 evaluates the sampled positions in double precision from the same float32 inputs (everything else unchanged)."""
    st = {k: np.array(v) for k, v in state.items()}
    percent_dense = float(st["percent_dense"])
    draws = np.asarray(draws, dtype=F32).reshape(-1, 3)
    taken, shapes = 0, []

    def draw(n):
        nonlocal taken
        shapes.append((int(n), 3))
        z = draws[taken:taken + n]
        assert z.shape[0] == n, "ran out of recorded draws"
        taken += n
        return z

    g, ga = quotient(st["xyz_gradient_accum"], st["denom"]), quotient(st["xyz_gradient_accum_abs"], st["denom"])
    with np.errstate(invalid="ignore"):
        ratio = (np.abs(g) >= F32(max_grad)).astype(F32).mean(dtype=F32)
    Q = quantile(ga, F32(1) - ratio)
    scale = exp32(st["scaling"])
    role, keep_idx, clone_idx, split_idx = select(st["xyz_gradient_accum"], st["xyz_gradient_accum_abs"], st["denom"], scale.max(axis=1), max_grad, Q,
                                                  percent_dense * extent)
    nc, ns = int(clone_idx.shape[0]), int(split_idx.shape[0])
    n0 = int(role.shape[0])
    xyz = st["xyz"].astype(pos_dtype)
    mag = np.zeros((n0, 3), dtype=np.float64)

    def append(new):
        nonlocal xyz, mag
        for name in PARAMS:
            if name != "xyz":
                st[name] = np.concatenate((st[name], new[name]), axis=0)
            for mom in ("m_", "v_"):
                st[mom + name] = np.concatenate((st[mom + name], np.zeros_like(new[name], dtype=F32)), axis=0)
        xyz = np.concatenate((xyz, new["xyz"]), axis=0)
        mag = np.concatenate((mag, new["mag"]), axis=0)

    # clone: one sample around each selected Gaussian, everything else copied
    new = {name: st[name][clone_idx] for name in PARAMS if name != "xyz"}
    new["xyz"], new["mag"] = sample_positions(st["xyz"][clone_idx], scale[clone_idx], st["rotation"][clone_idx], draw(nc), pos_dtype)
    append(new)
    # split: two samples around each selected Gaussian with scales shrunk by 1.6; the originals leave
    tile = lambda a: np.concatenate([a] * N_SPLIT, axis=0)          # noqa: E731
    new = {name: tile(st[name][split_idx]) for name in PARAMS if name != "xyz"}
    new["scaling"] = log32(tile(scale[split_idx]) / F32(0.8 * N_SPLIT))
    new["xyz"], new["mag"] = sample_positions(tile(st["xyz"][split_idx]), tile(scale[split_idx]), tile(st["rotation"][split_idx]),
                                              draw(N_SPLIT * ns), pos_dtype)
    append(new)
    stay = np.ones(n0 + nc + N_SPLIT * ns, dtype=bool)
    stay[split_idx] = False
    # prune (max_radii2D is all zeros by now)
    with np.errstate(invalid="ignore"):
        prune = _sigmoid(st["opacity"]).reshape(-1) < F32(min_opacity)
        if max_screen_size:
            big_vs = np.zeros_like(prune) if 0.0 <= max_screen_size else np.ones_like(prune)
            big_ws = exp32(st["scaling"]).max(axis=1) > F32(0.1 * extent)
            prune = prune | big_vs | big_ws
    n_pruned = int((prune & stay).sum())
    stay &= ~prune
    out = {"percent_dense": st["percent_dense"]}
    for name in PARAMS:
        out[name] = (xyz if name == "xyz" else st[name])[stay]
        out["m_" + name], out["v_" + name] = st["m_" + name][stay], st["v_" + name][stay]
    n_final = int(stay.sum())
    for name in STATS:
        out[name] = np.zeros((n_final, 1), dtype=F32)
    out["max_radii2D"] = np.zeros(n_final, dtype=F32)
    info = {"role": role, "keep_idx": keep_idx, "clone_idx": clone_idx, "split_idx": split_idx, "Q": Q, "mag": mag[stay],
            "sampled": (np.arange(stay.shape[0]) >= n0)[stay], "split_sample": (np.arange(stay.shape[0]) >= n0 + nc)[stay]}
    return out, (nc, ns, n_pruned), shapes, info


# ---- the recorded reference results (tests/golden/ref_densify_golden.npz, written by tests/golden/make_golden_densify.py) ----
def load_golden(path):
    """-> {case: dict(before, after, max_grad, min_opacity, extent, max_screen_size, ret, z, draw_shapes, xyz_f64, bound_ulp)}.
    bound_ulp: sampled positions are held to 8 ulp of |x| + sum_j |R_ij| |std_j z_j| around their float64 evaluation -- unless the
    reference itself was measured further out when the fixture was made, then to twice its recorded worst case."""
    z = np.load(path)
    cases = {}
    for case in [str(c) for c in z["cases"]]:
        pre = case + "."
        a = z[pre + "args"]
        worst = float(z[pre + "xyz_worst_ulp"])
        cases[case] = dict(before={k[len(pre) + 2:]: z[k] for k in z.files if k.startswith(pre + "b.")},
                           after={k[len(pre) + 2:]: z[k] for k in z.files if k.startswith(pre + "a.")},
                           max_grad=float(a[0]), min_opacity=float(a[1]), extent=float(a[2]), max_screen_size=None if np.isnan(a[3]) else int(a[3]),
                           ret=tuple(int(x) for x in z[pre + "ret"]), z=z[pre + "z"], draw_shapes=[tuple(int(x) for x in s) for s in z[pre + "draw_shapes"]],
                           xyz_f64=z[pre + "xyz_f64"], worst_ulp=worst, bound_ulp=8.0 if worst <= 8.0 else 2.0 * worst)
    return cases


def tie_categories(before, max_grad, extent):
    """the eight constructed edge categories of the tie case -> {name: rows of `before` in it}"""
    g, ga = quotient(before["xyz_gradient_accum"], before["denom"]), quotient(before["xyz_gradient_accum_abs"], before["denom"])
    accum, denom = before["xyz_gradient_accum"].reshape(-1), before["denom"].reshape(-1)
    with np.errstate(invalid="ignore"):
        ratio = (np.abs(g) >= F32(max_grad)).astype(F32).mean(dtype=F32)
    Q = quantile(ga, F32(1) - ratio)
    smax = exp32(before["scaling"]).max(axis=1)
    th = F32(float(before["percent_dense"]) * extent)
    mg = F32(max_grad)
    rows = lambda m: np.nonzero(m)[0]              # noqa: E731
    return {"quotient == max_grad": rows((g == mg) & (denom > 0)),
            "quotient one ulp below max_grad": rows(g == np.nextafter(mg, F32(0))),
            "grads_abs == Q": rows(ga == Q),
            "scale_max == threshold": rows(smax == th),
            "scale_max one ulp above threshold": rows(smax == np.nextafter(th, F32(np.inf))),
            "0 / 0 (NaN)": rows((denom == 0) & (accum == 0)),
            "x / 0 (inf)": rows((denom == 0) & (accum > 0)),
            "negative accum past max_grad": rows((accum < 0) & (np.abs(g) >= mg))}
