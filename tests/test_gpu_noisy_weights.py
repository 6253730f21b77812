"""GPU tests of ``sgw_noisy_weights`` (sorrel_amd/csrc/noisy.h): with ``eps_in`` the effective weights are NumPy's ``w + (s * eps)`` in every bit;
drawn, the normals are a function of their key alone, lie within 2^-16 of the float64 restatement (tests/noisy_common.py) and have a
normal's moments; backward mode is ``g * eps`` in every bit.  Every output lies between guard bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

from sorrel_amd import _native as N
from tests import learner_common as LK
from tests import noisy_common as NC

pytestmark = pytest.mark.gpu


def _dev(array, shift=4):
    """A device copy of a float32 array one element off 16 bytes (``shift`` bytes behind a 256-byte boundary), behind a guard."""
    g = LK.Guarded(torch, max(array.size, 1), np.float32, shift=shift)
    if array.size:
        g.buf[g.lo:g.lo + array.nbytes].copy_(torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1)))
    return g


def _call(d):
    N.launch("sgw_noisy_weights", d, torch.device(LK.DEV))
    torch.cuda.synchronize()


def _mixed(rng, count):
    """weight, sigma, eps with values whose product is inexact, and the contraction's tell-tale triple in element 0."""
    w = rng.standard_normal(count).astype(np.float32)
    s = (rng.standard_normal(count) * 0.3).astype(np.float32)
    e = rng.standard_normal(count).astype(np.float32)
    if count:
        w[0], s[0], e[0] = -1.0, 1.0 + 2.0 ** -12, 1.0 + 2.0 ** -12          # a fused multiply-add gives 2^-11 + 2^-24, two roundings 2^-11
    return w, s, e


def _forward_given(counts, seed, shifts=(4, 4, 4, 4, 4), out_eps=True):
    rng = np.random.default_rng(seed)
    host, dev, jobs = [], [], []
    for k, count in enumerate(counts):
        w, s, e = _mixed(rng, count)
        gw, gs, ge = _dev(w, shifts[0]), _dev(s, shifts[1]), _dev(e, shifts[2])
        go, gn = LK.Guarded(torch, max(count, 1), np.float32, shift=shifts[3]), LK.Guarded(torch, max(count, 1), np.float32, shift=shifts[4])
        host.append((w, s, e))
        dev.append((gw, gs, ge, go, gn))
        jobs.append(dict(weight=gw.ptr, sigma=gs.ptr, eps_in=ge.ptr, out_eff=go.ptr, out_eps=gn.ptr if out_eps else None, count=count, tensor_id=k))
    _call(NC.desc(N.NOISY_FORWARD, jobs))
    for k, (count, (w, s, e), (gw, gs, ge, go, gn)) in enumerate(zip(counts, host, dev)):
        ctx = (tuple(counts), k)
        for g in (gw, gs, ge, go, gn):
            assert g.intact(), ctx
        LK.same_bits(go.numpy()[:count], w + (s * e), "out_eff", ctx)
        if out_eps:
            LK.same_bits(gn.numpy()[:count], e, "out_eps", ctx)
        else:
            assert bool((gn.buf == 0xA5).all()), ctx
        if count == 0:
            assert bool((go.buf == 0xA5).all()), ctx
        for g, src in ((gw, w), (gs, s), (ge, e)):                       # the inputs are read only
            LK.same_bits(g.numpy()[:count], src, "input", ctx)


@pytest.mark.parametrize("count", NC.COUNTS)
def test_given_eps_one_job_every_bit(count):
    _forward_given([count], seed=count)


@pytest.mark.parametrize("jobs", [6, 18, N.NOISY_MAX_JOBS])
def test_given_eps_many_jobs_mixed_counts(jobs):
    counts = [(0, 1, 1025, 3, 0, 257, 4, 2049, 255, 5, 256, 0)[k % 12] for k in range(jobs)]
    _forward_given(counts, seed=jobs)


def test_trailing_and_leading_empty_jobs_write_nothing():
    _forward_given([0, 0, 7, 0, 0], seed=1)
    _forward_given([0, 0, 0], seed=2)


@pytest.mark.parametrize("which", range(5))
def test_each_pointer_one_element_off_sixteen_bytes(which):
    shifts = [0] * 5
    shifts[which] = 4
    _forward_given([1025, 5], seed=which, shifts=tuple(shifts))
    shifts[which] = 12
    _forward_given([257], seed=which + 10, shifts=tuple(shifts))


def test_out_eps_may_be_null():
    _forward_given([257, 3], seed=3, out_eps=False)


def test_non_finite_sigma_stays_in_its_element():
    count = 300
    rng = np.random.default_rng(5)
    w, s, e = _mixed(rng, count)
    s[7], s[100], s[299] = np.nan, np.inf, -np.inf
    e[100] = 0.0                                                            # inf * 0 = NaN
    gw, gs, ge = _dev(w), _dev(s), _dev(e)
    go = LK.Guarded(torch, count, np.float32, shift=4)
    _call(NC.desc(N.NOISY_FORWARD, [dict(weight=gw.ptr, sigma=gs.ptr, eps_in=ge.ptr, out_eff=go.ptr, count=count)]))
    with np.errstate(invalid="ignore"):
        want = w + (s * e)
    got = go.numpy()
    LK.same_bits(got, want, "out_eff")
    assert np.isnan(got[7]) and np.isnan(got[100]) and np.isinf(got[299]) and np.isfinite(np.delete(got, [7, 100, 299])).all()
    assert go.intact()


# ------------------------------------------------------------------------------------------------------------------ drawn
def _draw(key, count, tensor_jobs=None, position=0, total=1):
    """``(out_eff, out_eps, w, s)`` of one drawn job of ``count`` elements under ``key``, standing at ``position`` among ``total`` jobs (the
    others drawn too, with other ids and counts)."""
    seed, draw, tid = key
    rng = np.random.default_rng(count)
    w, s, _ = _mixed(rng, count)
    gw, gs = _dev(w), _dev(s)
    go, gn = LK.Guarded(torch, max(count, 1), np.float32, shift=4), LK.Guarded(torch, max(count, 1), np.float32, shift=4)
    mine = dict(weight=gw.ptr, sigma=gs.ptr, out_eff=go.ptr, out_eps=gn.ptr, count=count, tensor_id=tid)
    jobs, keep = [], [gw, gs, go, gn]
    for k in range(total):
        if k == position:
            jobs.append(mine)
            continue
        other = (5, 1025, 0, 300)[k % 4]
        a, b = _dev(np.ones(other, np.float32)), _dev(np.ones(other, np.float32))
        o = LK.Guarded(torch, max(other, 1), np.float32, shift=4)
        keep += [a, b, o]
        jobs.append(dict(weight=a.ptr, sigma=b.ptr, out_eff=o.ptr, count=other, tensor_id=100 + k))
    _call(NC.desc(N.NOISY_FORWARD, jobs, seed=seed, draw=draw))
    assert all(g.intact() for g in keep)
    return go.numpy()[:count], gn.numpy()[:count], w, s


@pytest.mark.parametrize("count", NC.COUNTS)
def test_drawn_normals_follow_the_definition(count):
    eff, eps, w, s = _draw(NC.BASE_KEY, count)
    want = NC.keyed_normals(*NC.BASE_KEY, count)
    worst = float(np.abs(eps.astype(np.float64) - want).max())
    print(count, "worst |eps - float64 restatement| =", worst)
    assert worst <= NC.EPS_CAP
    LK.same_bits(eff, w + (s * eps), "out_eff = w + s * out_eps")
    eff2, eps2, _, _ = _draw(NC.BASE_KEY, count)                           # the same key: the same bits
    LK.same_bits(eps2, eps, "a second call")
    LK.same_bits(eff2, eff, "a second call")


def test_seed_draw_and_tensor_id_change_the_draws():
    n = max(NC.COUNTS)
    _, base, _, _ = _draw(NC.BASE_KEY, n)
    for key in NC.OTHER_KEYS:
        _, other, _, _ = _draw(key, n)
        assert (other != base).mean() > 0.99, key
        assert float(np.abs(other.astype(np.float64) - NC.keyed_normals(*key, n)).max()) <= NC.EPS_CAP, key


def test_draws_do_not_depend_on_the_other_jobs_or_the_position():
    n = 1025
    _, alone, _, _ = _draw(NC.BASE_KEY, n)
    for position, total in ((0, 6), (5, 6), (3, 18), (N.NOISY_MAX_JOBS - 1, N.NOISY_MAX_JOBS)):
        _, among, _, _ = _draw(NC.BASE_KEY, n, position=position, total=total)
        LK.same_bits(among, alone, "out_eps", (position, total))


def test_a_million_draws_have_a_normals_moments():
    n = NC.STAT_COUNT
    seed, draw, tid = NC.STAT_KEY
    ws = torch.zeros((n,), dtype=torch.float32, device=LK.DEV)
    ones = torch.ones((n,), dtype=torch.float32, device=LK.DEV)
    out = LK.Guarded(torch, n, np.float32)
    eps = LK.Guarded(torch, n, np.float32)
    _call(NC.desc(N.NOISY_FORWARD, [dict(weight=ws.data_ptr(), sigma=ones.data_ptr(), out_eff=out.ptr, out_eps=eps.ptr, count=n, tensor_id=tid)],
                  seed=seed, draw=draw))
    x = eps.numpy().astype(np.float64)
    assert out.intact() and eps.intact()
    LK.same_bits(out.numpy(), eps.numpy() + np.float32(0.0), "0 + 1 * eps")
    mean_cap, var_cap = NC.stat_bounds(n)
    worst = float(np.abs(x - NC.keyed_normals(seed, draw, tid, n)).max())
    print("mean", x.mean(), "var", x.var(), "max", np.abs(x).max(), "worst |eps - float64 restatement| =", worst)
    assert abs(float(x.mean())) <= mean_cap
    assert abs(float(x.var()) - 1.0) <= var_cap
    assert float(np.abs(x).max()) <= NC.EPS_MAX
    assert worst <= NC.EPS_CAP


# ------------------------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("counts", [[c] for c in NC.COUNTS] + [[1025, 0, 3, 257, 1, 256]])
def test_backward_is_one_rounded_product(counts):
    rng = np.random.default_rng(sum(counts))
    host, dev, jobs = [], [], []
    for count in counts:
        g = rng.standard_normal(count).astype(np.float32)
        e = rng.standard_normal(count).astype(np.float32)
        gg, ge = _dev(g), _dev(e, 12)
        go = LK.Guarded(torch, max(count, 1), np.float32, shift=4)
        host.append((g, e))
        dev.append((gg, ge, go))
        jobs.append(dict(grad_eff=gg.ptr, eps_in=ge.ptr, out_grad_sigma=go.ptr, count=count))
    _call(NC.desc(N.NOISY_BACKWARD, jobs))
    for count, (g, e), (gg, ge, go) in zip(counts, host, dev):
        assert gg.intact() and ge.intact() and go.intact()
        LK.same_bits(go.numpy()[:count], g * e, "out_grad_sigma", tuple(counts))
        if count == 0:
            assert bool((go.buf == 0xA5).all())
