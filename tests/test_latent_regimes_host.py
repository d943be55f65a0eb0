"""CPU: the trained-regime input families of tests/latent_regimes.py are what their docstring says, and the precondition of
the tolerance rule of tests/test_gpu_latent_regimes.py holds for the estimator cases -- without a GPU."""
import math

import pytest
import torch

import latent_regimes as R


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("B,D", [(64, 10), (70, 1), (130, 17)])
def test_families_are_deterministic_and_in_the_stated_range(kind, B, D):
    a, b = R.family(kind, B, D, seed=5), R.family(kind, B, D, seed=5)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[1], R.family(kind, B, D, seed=6)[1])
    z, mu, logvar, eps = a
    assert all(t.shape == (B, D) and t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in a)
    assert torch.equal(z, mu + torch.exp(0.5 * logvar) * eps)
    A = R.n_active(D)
    assert A == max(1, D // 2) and A >= 1
    body = slice(4, None)                                   # rows without a hand-placed value in any family
    centre = -12.0 if kind == "sharp" else -9.0
    assert abs(logvar[body, :A].mean().item() - centre) < 0.3 and logvar[body, :A].max().item() < centre + 3.0
    assert mu[body, :A].abs().max().item() > 1.0            # cluster centres, units apart
    if D > A:
        assert mu[body, A:].abs().max().item() < 0.06 and logvar[body, A:].abs().max().item() < 0.12


@pytest.mark.parametrize("B,D", [(64, 10), (70, 1), (130, 17)])
def test_edges_rows_are_where_the_docstring_says(B, D):
    z, mu, logvar, eps = R.family("edges", B, D, seed=9)
    zt, mt, lt, et = R.family("trained", B, D, seed=9)
    A = R.n_active(D)
    for t in (z, mu, logvar, eps):
        assert torch.equal(t[0], t[1])                      # rows 0 and 1 tie
    assert bool((mu[2, :A] == 30.0).all())
    assert torch.equal(mu[2, A:], mt[2, A:]) and torch.equal(logvar[2], lt[2])
    assert logvar[3, D - 1].item() == 4.0
    if D > 1:
        assert logvar[3, 0].item() == -20.0
    assert torch.equal(mu[3], mt[3]) and torch.equal(logvar[3, 1:D - 1], lt[3, 1:D - 1])
    assert torch.equal(mu[4:], mt[4:]) and torch.equal(logvar[4:], lt[4:]) and torch.equal(eps[4:], et[4:])
    assert torch.equal(mu[0], mt[0]) and torch.equal(logvar[0], lt[0])


def test_ratio_and_bound():
    ref = torch.tensor([[100.0, 1e-3], [-50.0, 2e-3]], dtype=torch.double)
    got = ref + torch.tensor([[0.0, 1e-6], [0.0, 0.0]], dtype=torch.double)
    whole, _ = R.worst_ratio(got, ref, rtol=0.0, atol_rel=1e-5)
    per_dim, _ = R.worst_ratio(got, ref, rtol=0.0, atol_rel=1e-5, per_dim=True)
    assert whole == pytest.approx(1e-3) and per_dim == pytest.approx(50.0)          # the small column is no longer hidden
    assert R.worst_ratio(torch.tensor([float("nan")]), torch.tensor([1.0]), 1e-5, 1e-5)[0] == float("inf")
    assert R.bound(0.0) == 1.0 and R.bound(0.2) == 1.0 and R.bound(2.0) == 8.0


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("B,D,n_data", R.BTCVAE_SHAPES)
def test_fp32_oracle_stays_under_the_cap_for_the_estimator_cases(B, D, n_data, kind):
    """The rule's precondition for case 1: the reference's own fp32 arithmetic loses at most CAP x the stated tolerance on
    every output (forward row sums, per-dimension logsumexps, dz, dmu, dlv) against fp64, on the same fp32 inputs."""
    e32 = R.btcvae_e32(kind, B, D, n_data, True)
    print("e32 %s B=%d D=%d: %s" % (kind, B, D, ", ".join("%s %.3g" % kv for kv in e32.items())))
    for name, v in e32.items():
        assert math.isfinite(v) and v <= R.CAP, (name, v)


@pytest.mark.parametrize("B,D,n_data", [s for s in R.BTCVAE_SHAPES if s[1] > 1])
def test_rule_rejects_a_collapsed_dimension_error_the_whole_tensor_scale_hides(B, D, n_data):
    """dz of one collapsed dimension wrong by 1e-4 of that dimension's largest gradient (10 x the gradients' atol_rel): inside
    the whole-tensor tolerance of test_btcvae_fwd_bwd by orders of magnitude, outside max(1, 4 e32) of the per-dimension rule."""
    _, ref64, _ = R.btcvae_case("trained", B, D, n_data, True)
    e32 = R.btcvae_e32("trained", B, D, n_data, True)["dz"]
    d = D - 1
    assert d >= R.n_active(D)
    bad = ref64["dz"].clone()
    row = int(ref64["dz"][:, d].abs().argmin())
    bad[row, d] += 1e-4 * ref64["dz"][:, d].abs().max()
    whole, _ = R.worst_ratio(bad, ref64["dz"], **R.BTCVAE_BWD_TOL)
    per_dim, _ = R.worst_ratio(bad, ref64["dz"], per_dim=True, **R.BTCVAE_BWD_TOL)
    assert whole < 1e-2 and per_dim > R.bound(e32), (whole, per_dim, e32)


def test_fp32_oracle_stays_under_the_cap_without_stratified_weights():
    B, D, n_data = R.BTCVAE_SHAPES[0]
    for name, v in R.btcvae_e32("trained", B, D, n_data, False).items():
        assert math.isfinite(v) and v <= R.CAP, (name, v)
