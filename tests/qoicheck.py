"""float64 restatement of the rollout's quantities of interest (graph_trajectory.py:1042-1051 GNN_update "qoi", :221-242
volume('graph'), :244-256 qoi) and the element-wise bound the device accumulator is held to.

Layer k of a trajectory (its grains g, F = domain_factor, s = patch_size / mesh_size + 1, live = the mask after the step's
events, x = x_grain[:, 3:5] after the step's topology update and boundary step):
    A_k = sum_g live x[g, 0] / F^2          a_k[g] = live ? x[g, 0] s^2 / A_k : 0          e_k[g] = live x[g, 1] / 20 s^3
    V0 = 4 / (3 sqrt(pi)) a_0^1.5           T_k = T_{k-1} + dH / 2 (a_{k-1} + a_k), T_0 = 0
    volume_0 = V0,  volume_k = V0 + T_k + e_k (k >= 1)        dH = span (final_height - ini_height) / mesh_size / (frames - 1)
    size = cbrt(6 volume / pi) mesh_size;  d_mu, d_std (population) over ALL grains;  histogram over arange(0, 20, 1 or 2)

`variant` names a deliberate mistake (test_qoi.py proves the checks reject each of them):
    all_grains   the normalisation sums over all grains instead of the live ones
    no_F         the domain factor left out of A_k
    rectangle    T_k = T_{k-1} + dH a_k instead of the trapezoid
    e_summed     e_k accumulated over the layers instead of added per layer
    one_union    a union normalised as one trajectory
    no_span      dH without the span
"""
import numpy as np

VARIANTS = ("all_grains", "no_F", "rectangle", "e_summed", "one_union", "no_span")


def delta_h(span, mesh_size, ini_height, final_height, frames):
    return span * (final_height - ini_height) / mesh_size / (frames - 1)


def frames_default(ini_height, final_height):
    return int((final_height - ini_height) / 0.4) + 1   # test.py:191, 307


def restate(xg34, mask, *, patch_size, mesh_size, ini_height, final_height, frames, span, domain_factor=1.0, offsets=None,
            area0=None, variant=None):
    """xg34 [L+1, N, 2] (the float32 features, taken to float64 as the reference's numpy does), mask
    [L+1, N].  Returns float64 [L+1, N] arrays `area_traj`, `extraV_traj`, `T`, `volume_traj` and, for the element-wise
    bound, `T_terms` / `volume_terms` = the sums of the absolute values of the terms each element is made of."""
    assert variant is None or variant in VARIANTS, variant
    x32 = np.asarray(xg34, np.float32)
    x = x32.astype(np.float64)
    live = np.asarray(mask) > 0
    L1, N = live.shape
    off = np.asarray([0, N] if offsets is None or variant == "one_union" else offsets, np.int64)
    F = 1.0 if variant == "no_F" else float(domain_factor)
    s = patch_size / mesh_size + 1
    dH = delta_h(1 if variant == "no_span" else span, mesh_size, ini_height, final_height, frames)
    a, e = np.zeros((L1, N)), np.zeros((L1, N))
    for k in range(L1):
        for lo, hi in zip(off[:-1], off[1:]):
            m = live[k, lo:hi]
            if not m.any():
                continue   # (all zeros, no division)
            A = (x[k, lo:hi, 0] if variant == "all_grains" else x[k, lo:hi, 0] * m).sum() / F ** 2
            # (`area*s**2` there is a float32 scalar times a Python float: a float32 product under NumPy 2's promotion
            #  rules, with which the goldens were made; everything else is float64)
            a[k, lo:hi] = np.where(m, (x32[k, lo:hi, 0] * np.float32(s ** 2)).astype(np.float64) / A, 0.0)
        e[k] = live[k] * x[k, :, 1] / 20 * s ** 3
    if area0 is not None:
        a[0] = np.asarray(area0, np.float64)
    V0 = 4 / 3 / np.sqrt(np.pi) * a[0] ** 1.5
    T, T_terms = np.zeros((L1, N)), np.zeros((L1, N))
    vol, vol_terms = np.zeros((L1, N)), np.zeros((L1, N))
    vol[0], vol_terms[0] = V0, np.abs(V0)
    for k in range(1, L1):
        if variant == "rectangle":
            T[k] = T[k - 1] + dH * a[k]
        else:
            T[k] = T[k - 1] + dH * a[k - 1] / 2 + dH * a[k] / 2
        T_terms[k] = T_terms[k - 1] + np.abs(dH * a[k - 1] / 2) + np.abs(dH * a[k] / 2)
        ek = e[1:k + 1].sum(0) if variant == "e_summed" else e[k]
        vol[k] = V0 + T[k] + ek
        vol_terms[k] = np.abs(V0) + T_terms[k] + np.abs(e[k])
    return {"area_traj": a, "extraV_traj": e, "T": T, "volume_traj": vol, "T_terms": T_terms, "volume_terms": vol_terms,
            "V0": V0}


def statistics(volume, mesh_size, offsets=None):
    """(size, [d_mu], [d_std], [counts], [density], [edges]) of the last layer's volumes, per trajectory."""
    volume = np.asarray(volume, np.float64)
    off = np.asarray([0, volume.size] if offsets is None else offsets, np.int64)
    size = np.cbrt(6 * volume / np.pi) * mesh_size
    mu, std, counts, dens, edges = [], [], [], [], []
    for lo, hi in zip(off[:-1], off[1:]):
        bins = np.arange(0, 20, 1 if hi - lo > 400 else 2)
        mu.append(np.mean(size[lo:hi]))
        std.append(np.std(size[lo:hi]))
        counts.append(np.histogram(size[lo:hi], bins)[0])
        dens.append(np.histogram(size[lo:hi], bins, density=True)[0])
        edges.append(bins)
    return size, mu, std, counts, dens, edges


RTOL_TERMS = 1e-5   # |got - ref64| <= 1e-5 * sum |terms of that element|


def excess(got, ref, terms):
    """Worst |got - ref| / (RTOL_TERMS * terms) over the elements (0 where both the difference and the terms are 0;
    inf where an element differs although it has no term, or is not finite); <= 1 passes."""
    got, ref, terms = (np.asarray(v, np.float64) for v in (got, ref, terms))
    assert got.shape == ref.shape == terms.shape, (got.shape, ref.shape, terms.shape)
    diff = np.abs(got - ref)
    diff[~np.isfinite(got)] = np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(diff == 0, 0.0, diff / (RTOL_TERMS * terms))
    return float(ratio.max()) if ratio.size else 0.0


def golden_kwargs(d):
    """The constants a golden file of tests/golden/make_golden_qoi.py carries, as restate()'s keywords."""
    return dict(patch_size=float(d["patch_size"]), mesh_size=float(d["mesh_size"]), ini_height=float(d["ini_height"]),
                final_height=float(d["final_height"]), frames=int(d["frames"]), span=int(d["span"]),
                domain_factor=float(d["lxd"]) / float(d["patch_size"]))
