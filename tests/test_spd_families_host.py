"""tests/spd_families.py on the host: what the generators produce, and that the factor comparison of the GPU tests
(tests/test_gpu_dense_generic.py) can see a wrong ROW inside an off-diagonal block -- which no assertion can on the volatility
kernel, whose factor has rank-one blocks.  No GPU."""
import numpy as np
import pytest

import spd_families as F

N, B = 300, 2
BLK = (slice(128, 256), slice(0, 128))                 # a whole off-diagonal 128-block of a 300 x 300 factor
_CACHE = {}


def _family(name):
    if name not in _CACHE:
        A = F.make(name, B, N, np.float32, seed=3)
        _CACHE[name] = (A, np.linalg.cholesky(A))
    return _CACHE[name]


@pytest.mark.parametrize("name", F.FAMILIES)
def test_generators_are_seeded_symmetric_and_exact_in_the_target_dtype(name):
    A, _L = _family(name)
    assert A.dtype == np.float64 and A.shape == (B, N, N)
    assert np.array_equal(A, np.swapaxes(A, -1, -2))
    assert np.array_equal(A, A.astype(np.float32).astype(np.float64))
    assert np.array_equal(A, F.make(name, B, N, np.float32, seed=3))
    assert not np.array_equal(A, F.make(name, B, N, np.float32, seed=4))
    assert not np.array_equal(A[0], A[1])
    A64 = F.make(name, B, N, np.float64, seed=3)
    assert not np.array_equal(A64, A) and np.abs(A64 - A).max() <= 2.0 ** -24 * np.abs(A).max()
    r = F.rhs(B, N, np.float32, seed=3)
    assert r.shape == (B, N) and np.array_equal(r, r.astype(np.float32).astype(np.float64))


def test_condition_numbers_are_the_regimes_the_tolerances_are_stated_for():
    cond = {name: np.linalg.cond(_family(name)[0]) for name in F.GENERIC}
    assert (cond["wishart"] > 3).all() and (cond["wishart"] < 8).all(), cond
    assert (cond["rbf_irregular"] > 5e2).all() and (cond["rbf_irregular"] <= 3e3).all(), cond
    assert (cond["scaled"] > 1e5).all() and (cond["scaled"] < 1e7).all(), cond
    # (rbf_irregular's largest eigenvalue grows like the density of points, N 0.3 sqrt(2 pi) / 4: cond ~ 3.8 N)
    assert (np.linalg.cond(F.rbf_irregular(1, 640, np.float32, seed=0)) <= 3e3).all()


def test_rank_of_an_off_diagonal_block_of_the_factor():
    """The gap: the volatility kernel's factor has ONE free number per column below the diagonal."""
    rank = {name: [F.block_rank(_family(name)[1][b][BLK]) for b in range(B)] for name in F.FAMILIES}
    assert rank["wishart"] == [128] * B and rank["scaled"] == [128] * B, rank
    assert min(rank["rbf_irregular"]) > 1, rank
    assert rank["vol"] == [1] * B, rank
    Lv = _family("vol")[1]
    for j in (0, 64, 127):                             # a column of it below the diagonal is constant
        col = Lv[:, j + 1:, j]
        assert np.abs(col / col[:, :1] - 1).max() < 1e-12


@pytest.mark.parametrize("name", F.FAMILIES)
def test_helper_accepts_an_fp32_lapack_factor(name):
    """The reference's own fp32 error sits well inside the fixed tolerance (2e-5 on the row-normalised measure)."""
    A, L = _family(name)
    L32 = np.linalg.cholesky(A.astype(np.float32))
    assert L32.dtype == np.float32
    err = F.assert_factor_close(L32, L, A, 2e-5, name)
    assert 0 < err < 5e-6, err
    assert F.factor_error(L, L, A) == 0.0


@pytest.mark.parametrize("name", F.GENERIC)
def test_helper_rejects_rows_permuted_inside_an_off_diagonal_block(name):
    A, L = _family(name)
    for perm in (np.roll(np.arange(128), 1), np.arange(128)[::-1], np.r_[np.arange(12), np.roll(np.arange(12, 122), 1), np.arange(122, 128)]):
        bad = F.permute_block_rows(L, *BLK, perm)
        assert not np.array_equal(bad, L) and np.array_equal(np.sort(bad, axis=1), np.sort(L, axis=1))   # the same numbers
        assert F.factor_error(bad, L, A) > 1e-3        # far beyond any fp32 tolerance, not marginally
        with pytest.raises(AssertionError):
            F.assert_factor_close(bad, L, A, 2e-5, name)
    nan = L.copy()
    nan[1, 200, 5] = np.nan
    with pytest.raises(AssertionError):
        F.assert_factor_close(nan, L, A, 2e-5, name)


def test_helper_rejects_a_swap_at_every_row_scale_of_scaled():
    """`scaled` has rows from 10^-1.5 to 10^1.5: two exchanged rows are seen wherever they sit, because every entry's error is
    taken relative to its own row's norm sqrt(A_ii)."""
    A, L = _family("scaled")
    row = np.sqrt(np.diagonal(A, axis1=-2, axis2=-1))
    assert row[:, 128:256].max() / row[:, 128:256].min() > 300
    for i in range(127):
        perm = np.arange(128)
        perm[[i, i + 1]] = perm[[i + 1, i]]
        bad = F.permute_block_rows(L, *BLK, perm)
        assert F.factor_error(bad, L, A) > 1e-3, (i, row[:, 128 + i])


def test_helper_accepts_the_same_permutations_on_the_volatility_kernel():
    """The control: on K[i,j] = V[min(i,j)] + sigma^2 I a tile may take any row of the block for any other."""
    A, L = _family("vol")
    for perm in (np.roll(np.arange(128), 1), np.arange(128)[::-1]):
        bad = F.permute_block_rows(L, *BLK, perm)
        assert F.assert_factor_close(bad, L, A, 2e-5, "vol") < 1e-12


def test_reference_quantities_are_consistent():
    A = F.make("wishart", 2, 150, np.float32, seed=1)
    r = F.rhs(2, 150, np.float32, seed=1)
    ref = F.reference(A, r, keep_y=True)
    Ai = np.linalg.inv(A)
    assert np.allclose(ref["alpha"], np.einsum("bij,bj->bi", Ai, r), rtol=1e-10, atol=1e-12)
    assert np.allclose(ref["trinv"], np.trace(Ai, axis1=-2, axis2=-1), rtol=1e-10)
    assert np.allclose(ref["logdet"], np.linalg.slogdet(A)[1], rtol=1e-10)
    assert np.allclose(ref["quad"], (r * ref["alpha"]).sum(-1), rtol=1e-10)
    assert np.allclose(ref["Y"] @ np.swapaxes(ref["Y"], -1, -2), Ai, rtol=1e-9, atol=1e-12)
