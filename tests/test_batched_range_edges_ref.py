"""The float64 restatements of the batched families (mi355x_qr.h sections 8c to 8n) at the edges of the double range, on the inputs
tests/test_gpu_batched_range_edges.py runs the kernels on (tests/batched_edge_ref.py has the inputs, the scale pairs and what de-scales
each output).  No GPU.

For every family and every admissible scale pair the restatement runs unscaled and scaled: every integer output (info, status, iteration,
elimination, solve and sweep counts, states, ranks, accepted, nfev, njev, par_status, pegs) equals the unscaled run's, every floating
output is finite and, de-scaled by the exact power of two, within 1e-9 (relative, per member) of the unscaled run's.  This is what lets
the GPU file demand the unscaled run's decisions of the kernels at every scale, and it is the regression test of the gradient norm of the
trust-region search: batched_trust_ref.gradient_norm restates bt_wave_gnorm of csrc/qr_batched_trust_dev.h, and the two members of the
defect's report are here by name.  It is also the regression test of the column norm of the Householder step (hp_ref.column_scale
restates qb_wave_nrm of csrc/qr_batched_dev.h): batched_edge_ref.svd_ref asserts the section's four bounds at every pair.
"""
import numpy as np
import pytest

import batched_edge_ref as E
import batched_lm_ref as L
import batched_trust_ref as T
import batched_update_ref as UP
import hp_ref as H


def _sweep(ref, pairs, *args):
    base = ref(*args, 0, 0)
    for pair in pairs:
        E.compare(base, ref(*args, *pair), (ref.__name__,) + args + (E.tag(pair),))


# ------------------------------------------------------------------------------------------------
# the gradient norm of the search (8g, and through it 8m and 8n)
# ------------------------------------------------------------------------------------------------
def test_gradient_norm_is_the_plain_sum_inside_the_window_and_right_outside_it():
    g = T.D.U(11, 31)
    plain = lambda v: np.sqrt((v * v).sum())
    for e in (0, 1, -1, 100, -100, T.G_WINDOW - 1, -(T.G_WINDOW - 2)):
        s = E.p2(e)
        assert T.gradient_norm(s * g) == plain(s * g), e                     # bitwise what the search always formed
    for e in (T.G_WINDOW + 1, 300, 480, 600, 960, -T.G_WINDOW, -300, -480, -600, -960):
        s = E.p2(e)
        assert T.gradient_norm(s * g) == s * plain(g), e                     # exact: the scaling inside is by a power of two
    assert T.gradient_norm(np.zeros(5)) == 0.0 and T.gradient_norm(np.zeros(0)) == 0.0
    assert T.gradient_norm(E.p2(700) * np.array([3.0, 4.0])) == E.p2(700) * 5.0    # representable, though its square is not
    assert T.gradient_norm(E.p2(-700) * np.array([3.0, 4.0, 0.0])) == E.p2(-700) * 5.0
    assert T.gradient_norm(np.array([5e-324, 0.0])) == 5e-324                # the smallest subnormal
    assert np.isinf(T.gradient_norm(np.array([np.inf, 1.0]))) and np.isnan(T.gradient_norm(np.array([np.nan, 1.0])))     # as before


@pytest.mark.parametrize("e", [300, 480, -300, -480])
def test_named_rank_deficient_member_scaled_with_its_right_hand_side(e):
    """(R, z) both times 2^e, R(4, 4) == 0, Delta = 0.5, rtol = 1e-3: before the fix the squares of g overflowed from 2^300 on, gnorm was
    inf, parl = 0 made bt_start take par = inf: 10 eliminations, status 3, lambda = inf, |D x| = NaN beside info == 0"""
    R, z = E.named_rank_deficient()
    base = T.lmpar(R, z, 0.5, rtol=1e-3)
    assert (base["iter"], base["status"], base["info"]) == (3, 0, 0) and base["lam"] == 1.0302484309130067
    s = E.p2(e)
    o = T.lmpar(s * R, s * z, 0.5, rtol=1e-3)
    assert (o["iter"], o["status"], o["info"]) == (3, 0, 0)
    assert np.isfinite(o["lam"]) and np.isfinite(o["xnorm"]) and np.isfinite(o["X"]).all() and np.isfinite(o["resid"])
    assert abs(o["lam"] / s - base["lam"]) <= E.RTOL * base["lam"] and abs(o["xnorm"] - base["xnorm"]) <= E.RTOL * base["xnorm"]
    assert np.max(np.abs(o["X"] - base["X"])) <= E.RTOL * np.max(np.abs(base["X"]))


@pytest.mark.parametrize("e", [300, 480, -300, -480])
@pytest.mark.parametrize("m,n", [(64, 31), (40, 33)])
def test_named_full_rank_members_take_the_unscaled_runs_eliminations(m, n, e):
    """(R, z) both times 2^e, every Delta fraction and both rtol: before the fix the squares of g went to 0 at 2^-300, gnorm was 0, paru
    fell to DBL_MIN / min(Delta, 0.1), and the search took one elimination more (64 x 31, member 0, fraction 0.01: 3 instead of 2)"""
    A, b, d = T.batch(m, n, 5)
    s = E.p2(e)
    for q in range(5):
        R, z, rss = T.factors(A[q], b[q])
        gn = T.gauss_newton_dxnorm(R, z, d[q])
        for frac in T.FRACS:
            for rtol in T.RTOLS:
                base = T.lmpar(R, z, frac * gn, d[q], rss=rss, rtol=rtol)
                o = T.lmpar(s * R, s * z, frac * gn, d[q], rss=s * s * rss, rtol=rtol)
                assert (o["iter"], o["status"], o["info"]) == (base["iter"], base["status"], 0), (q, frac, rtol, o["iter"], base["iter"])
                assert np.isfinite(o["lam"]) and abs(o["lam"] / s - base["lam"]) <= E.RTOL * base["lam"], (q, frac, rtol)
    if (m, n) == (64, 31):
        R, z, rss = T.factors(A[0], b[0])
        assert T.lmpar(R, z, 0.01 * T.gauss_newton_dxnorm(R, z, d[0]), d[0], rss=rss, rtol=0.1)["iter"] == 2


def test_lm_search_is_the_trust_search():
    """batched_lm_ref.search carries the same gradient norm: par = lambda^2 of batched_trust_ref.lmpar on the named member at 2^300"""
    R, z = E.named_rank_deficient()
    s = E.p2(300)
    a = T.lmpar(s * R, s * z, 0.5, np.ones(7), rtol=1e-3)
    c = L.search(s * R, s * z, 0.5, np.ones(7), None, 0.0, 1e-3, T.MAXIT)
    assert (c["iter"], c["status"], c["info"]) == (a["iter"], a["status"], 0) == (3, 0, 0)
    assert np.sqrt(c["par"]) == a["lam"] and np.array_equal(c["X"], a["X"]) and c["xnorm"] == a["xnorm"]


# ------------------------------------------------------------------------------------------------
# every family at every admissible pair
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.TRUST_ORDERS)
def test_trust(n):
    p = E.trust_inputs(n)
    base = E.trust_ref(p, 0, 0)
    assert base[0]["iter"].max() >= 2 and base[0]["iter"][E.TRUST_ZERO] >= 2 and sorted(set(base[0]["status"])) == [0, 1]
    for pair in E.PAIRS:
        E.compare(base, E.trust_ref(p, *pair), ("trust", n, E.tag(pair)))


@pytest.mark.parametrize("bounded", [False, True], ids=["lm", "lmb"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("which", ["wave", "workgroup", "nonlinear"])
def test_lm_and_bounded_lm(which, mode, bounded):
    case = E.lm_nonlinear(bounded) if which == "nonlinear" else E.lm_linear(*E.LM_SHAPES[which == "workgroup"])
    base = E.lm_ref(case, 0, mode, bounded)
    assert not base[0]["info"].any() and (base[0]["status"] > 0).all() and base[0]["nfev"].min() >= 3
    if bounded:
        assert (base[0]["peg"] != 0).any(axis=1).all(), "a bound is active at the end of every member"
    for pair in E.JOINT:
        E.compare(base, E.lm_ref(case, pair[0], mode, bounded), ("lmb" if bounded else "lm", which, mode, E.tag(pair)))


@pytest.mark.parametrize("shape", E.DAMPED_SHAPES)
def test_damped(shape):
    _sweep(E.damped_ref, E.PAIRS, shape)


@pytest.mark.parametrize("shape", E.DAMPED_WIDE)
def test_damped_wide(shape):
    _sweep(E.damped_wide_ref, E.PAIRS, shape)


@pytest.mark.parametrize("n", E.DAMPED_TRI)
def test_damped_from_pivoted_factors_with_a_zero_column(n):
    _sweep(E.damped_tri_ref, E.PAIRS, n)


@pytest.mark.parametrize("shape", E.BVLS_SHAPES)
def test_bvls(shape):
    _sweep(E.bvls_ref, E.PAIRS, shape)


@pytest.mark.parametrize("shape", E.LSEI_SHAPES)
def test_lsei(shape):
    _sweep(E.lsei_ref, E.PAIRS, shape)


@pytest.mark.parametrize("shape", E.LSE_SHAPES)
def test_gglse(shape):
    _sweep(E.lse_ref, E.PAIRS, shape)


@pytest.mark.parametrize("loss", E.IRLS_LOSSES, ids=["huber", "bisquare"])
@pytest.mark.parametrize("shape", E.IRLS_SHAPES)
def test_irls(shape, loss):
    _sweep(E.irls_ref, E.PAIRS, shape, loss)


@pytest.mark.parametrize("shape", E.STATS_SHAPES)
def test_fit_stats(shape):
    _sweep(E.stats_ref, E.PAIRS, shape)


@pytest.mark.parametrize("n", E.STATS_TRI)
def test_covariance_from_a_triangle_of_rank_n_minus_1(n):
    base = E.tri_ref(n, 0)
    for pair in E.SVD_PAIRS:
        E.compare(base, E.tri_ref(n, pair[0]), ("covar", n, E.tag(pair)))


@pytest.mark.parametrize("shape", E.MINNORM_SHAPES)
def test_minnorm(shape):
    _sweep(E.minnorm_ref, E.PAIRS, shape)


@pytest.mark.parametrize("shape", E.SVD_SHAPES)
def test_svd(shape):
    base = E.svd_ref(shape, 0)
    assert base[0]["rank"].tolist() == [shape[1]] * 2 + [shape[1] - 2] + [shape[1]] * 2
    for pair in E.SVD_PAIRS:
        E.compare(base, E.svd_ref(shape, pair[0]), ("svd", shape, E.tag(pair)))


@pytest.mark.parametrize("shape", E.UPDATE_SHAPES)
def test_update_and_accumulator(shape):
    _sweep(E.update_ref, E.PAIRS, shape)
    _sweep(E.acc_ref, E.PAIRS, shape)
    assert not E.acc_ref(shape, 0, 0)[0]["info"].any()
    # the rule of tests/test_gpu_batched_update.py for an input: the float64 restatement stays within half of each of its three bounds
    c = E.update_inputs(*shape)
    fl = E.update_ref(shape, 0, 0)[1]
    for q in range(E.BATCH):
        Rld = UP.update(c["R"][q], c["B"][q], c["p_add"], dtype=H.LD)[0]
        r = UP.measures(c["n"], c["p_add"], dict(R=c["R"][q], B=c["B"][q], C1=c["Z"][q], C2=c["C2"][q]), fl["R"][q], fl["C1"][q], fl["C2"][q], Rld)
        assert max(r) <= 0.5, (q, r)
