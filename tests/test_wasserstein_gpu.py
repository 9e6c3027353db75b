"""es_wasserstein_1d (csrc/wasserstein.hip) against scipy.stats.wasserstein_distance.

Bound: |got - ref| <= 2 (nu + nv) 2^-52 ref.  The kernel and scipy sum the same non-negative fp64 terms
(scipy's _cdf_distance with p = 1: |cu/nu - cv/nv| (a[k+1] - a[k]) over the jointly sorted values) in
different orders; each order errs by at most (m - 1) 2^-53 relative, m = nu + nv - 1 terms.  A reference
of 0 must give exactly 0.  The sizes sit on both sides of every power of two the bitonic network pads
to, on both sides of hip.WS_LDS_MAX (LDS sort / global-memory passes), and one spans several LDS tiles.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def wasserstein_distance(u, v):
    """scipy's, imported at first use: a module-level scipy import would run at collection, for every
    run of the suite, and its tens of thousands of long-lived objects change when the cyclic garbage
    collector runs in the tests collected before this file."""
    from scipy.stats import wasserstein_distance as ref
    return ref(u, v)


def _data(nu, nv, ties=False, seed=0):
    rng = np.random.default_rng(seed)
    u, v = rng.gamma(2.0, 300.0, nu), rng.gamma(2.2, 280.0, nv)
    if ties:
        u, v = np.round(u), np.round(v)
        u[:nu // 3] = 0.0
        v[:nv // 4] = 0.0
    return u, v


def _check(got, ref, m, what=""):
    err = abs(got - ref)
    bound = 2 * m * 2.0 ** -52 * ref
    print(f"ws {what}: got {got!r} ref {ref!r} err {err:.3e} bound {bound:.3e}")
    if ref == 0:
        assert got == 0.0, what
    else:
        assert err <= bound, what


def _lds_max():
    from expertsim import hip
    return hip.WS_LDS_MAX


def _sizes():
    # "lds": nu + nv == hip.WS_LDS_MAX (+ 1), resolved in the test; the last is the largest supported problem
    return [(1, 1, False), (1, 7, False), (40, 40, False), (37, 61, True), (63, 65, False), (64, 64, False),
            (65, 63, False), (255, 257, False), (1024, 1023, False), ("lds", "lds", False), ("lds", "lds+1", False),
            (20000, 12768, True), (2 ** 19, 2 ** 19, False)]


@pytest.mark.parametrize("nu,nv,ties", _sizes())
def test_single_segment_matches_scipy(nu, nv, ties):
    from expertsim.train.utils import wasserstein_1d_device
    if nu == "lds":
        L = _lds_max()
        nu, nv = L // 2, L - L // 2 + (1 if nv == "lds+1" else 0)
        assert nu + nv in (L, L + 1)
    u, v = _data(nu, nv, ties, seed=nu + 3 * nv)
    ud, vd = torch.from_numpy(u[:, None]).to(DEV), torch.from_numpy(v[:, None]).to(DEV)
    got = wasserstein_1d_device(ud, vd)
    assert got.shape == (1, 1) and got.dtype == torch.float64 and got.is_cuda
    _check(float(got[0, 0]), wasserstein_distance(u, v), nu + nv, f"({nu}, {nv})")


def test_all_values_equal_gives_zero():
    from expertsim.train.utils import wasserstein_1d_device
    u = torch.full((2, 1), 417.25, dtype=torch.float64, device=DEV)
    got = wasserstein_1d_device(u, u.clone())
    assert float(got[0, 0]) == 0.0


def _dispatch(expert, E):
    from expertsim import hip
    n = expert.numel()
    perm = torch.empty(n, dtype=torch.int32, device=DEV)
    offs = torch.empty(E + 1, dtype=torch.int32, device=DEV)
    hip.call("es_router_dispatch", hip.ptr(expert), n, E, hip.ptr(perm), hip.ptr(offs), hip.stream_ptr())
    return perm, offs


def test_multi_segment_strided_with_an_empty_expert():
    from expertsim.train.utils import wasserstein_1d_device
    N, Cn, E = 96, 5, 4
    rng = np.random.default_rng(5)
    ub, vb = rng.gamma(2.0, 300.0, (N, 7)), rng.gamma(2.2, 280.0, (N, 7))
    expert = rng.choice([0, 1, 3], size=N).astype(np.int32)          # expert 2 has no rows
    ud, vd = torch.from_numpy(ub).to(DEV)[:, :Cn], torch.from_numpy(vb).to(DEV)[:, :Cn]
    assert ud.stride(0) == 7
    perm, offs = _dispatch(torch.from_numpy(expert).to(DEV), E)
    seg = torch.empty(E + 1, 2, dtype=torch.int32, device=DEV)
    seg[0, 0], seg[0, 1] = 0, N
    seg[1:, 0], seg[1:, 1] = offs[:-1], offs[1:]
    got = wasserstein_1d_device(ud, vd, seg, seg, perm, perm).cpu().numpy()
    assert got.shape == (E + 1, Cn)
    for s in range(E + 1):
        rows = np.arange(N) if s == 0 else np.where(expert == s - 1)[0]
        for c in range(Cn):
            if len(rows) == 0:
                assert got[s, c] == 0.0
            else:
                _check(got[s, c], wasserstein_distance(ub[rows, c], vb[rows, c]), 2 * len(rows), f"seg {s} ch {c}")
    assert np.all(got[3] == 0.0) and np.all(got[[0, 1, 2, 4]] > 0)


def test_unequal_sides_of_a_segment():
    from expertsim.train.utils import wasserstein_1d_device
    u, v = _data(64, 64, seed=9)
    ud, vd = torch.from_numpy(u[:, None]).to(DEV), torch.from_numpy(v[:, None]).to(DEV)
    u_seg = torch.tensor([[0, 10], [3, 64]], dtype=torch.int32, device=DEV)
    v_seg = torch.tensor([[5, 40], [60, 64]], dtype=torch.int32, device=DEV)
    got = wasserstein_1d_device(ud, vd, u_seg, v_seg).cpu().numpy()
    _check(got[0, 0], wasserstein_distance(u[0:10], v[5:40]), 45, "u[0:10] v[5:40]")
    _check(got[1, 0], wasserstein_distance(u[3:64], v[60:64]), 65, "u[3:64] v[60:64]")


def _raw_call(ud, vd, n_seg, u_cap, v_cap, out, work, work_bytes, check=True):
    from expertsim import hip
    seg_u = torch.tensor([[0, ud.shape[0]]] * n_seg, dtype=torch.int32, device=DEV)
    seg_v = torch.tensor([[0, vd.shape[0]]] * n_seg, dtype=torch.int32, device=DEV)
    args = (hip.ptr(ud), ud.stride(0), ud.shape[0], None, hip.ptr(seg_u), hip.ptr(vd), vd.stride(0), vd.shape[0],
            None, hip.ptr(seg_v), n_seg, ud.shape[1], u_cap, v_cap, hip.ptr(out), hip.ptr(work), work_bytes,
            hip.stream_ptr())
    if check:
        return hip.call("es_wasserstein_1d", *args)
    return hip.lib().es_wasserstein_1d(*args)


@pytest.mark.parametrize("nu,nv", [(300, 211), (5000, 4001)])     # LDS path, global-memory path
def test_nan_prefill_tail_untouched_and_bitwise_rerun(nu, nv):
    from expertsim import hip
    u, v = _data(nu, nv, ties=True, seed=21)
    ud = torch.from_numpy(np.stack([u, u[::-1] * 0.5], 1)).to(DEV)
    vd = torch.from_numpy(np.stack([v, v + 3.0], 1)).to(DEV)
    n_seg, Cn = 2, 2
    need = int(hip.lib().es_wasserstein_1d_workspace(n_seg, Cn, nu, nv))
    assert (need > 0) == (nu + nv > hip.WS_LDS_MAX)
    outs = []
    for _ in range(2):
        out = torch.full(((n_seg + 1) * Cn,), float("nan"), dtype=torch.float64, device=DEV)
        work = torch.full((max(need, 8) // 8 + 1,), float("nan"), dtype=torch.float64, device=DEV)
        _raw_call(ud, vd, n_seg, nu, nv, out, work, work.numel() * 8)
        outs.append(out.cpu().numpy())
    a, b = outs
    assert np.all(np.isfinite(a[:n_seg * Cn])) and np.all(np.isnan(a[n_seg * Cn:]))
    assert a[:n_seg * Cn].tobytes() == b[:n_seg * Cn].tobytes()
    assert a[0] == a[2] and a[1] == a[3]                              # both segments cover the same rows
    _check(a[0], wasserstein_distance(u, v), nu + nv, "col 0")
    _check(a[1], wasserstein_distance(u[::-1] * 0.5, v + 3.0), nu + nv, "col 1")


def test_argument_errors_do_not_launch():
    from expertsim import hip
    nu, nv = 5000, 4001
    u, v = _data(nu, nv, seed=2)
    ud, vd = torch.from_numpy(u[:, None]).to(DEV), torch.from_numpy(v[:, None]).to(DEV)
    need = int(hip.lib().es_wasserstein_1d_workspace(1, 1, nu, nv))
    assert need >= (nu + nv) * 9
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert _raw_call(ud, vd, 1, nu, nv, out, work, need - 1, check=False) == 1          # ES_ERR_ARG
    assert b"workspace" in hip.lib().es_last_error()
    with pytest.raises(hip.HipError):
        _raw_call(ud, vd, 1, nu, nv, out, None, 0)
    with pytest.raises(hip.HipError):
        _raw_call(ud, vd, 1, 2 ** 19, 2 ** 19 + 1, out, work, need)                   # u_cap + v_cap > 2^20
    assert hip.lib().es_wasserstein_1d_workspace(1, 1, 2 ** 19, 2 ** 19 + 1) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    _raw_call(ud, vd, 1, nu, nv, out, work, need)                                      # and the good call works
    _check(float(out[0]), wasserstein_distance(u, v), nu + nv, "after errors")
