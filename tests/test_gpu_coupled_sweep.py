"""The coupled triangular sweep (kernels_trsv.hip): H_k = Inv_k^T L[k+1,k]^T and G_k = Inv_k L[k,k-1] are multiplied
out once per factorisation (beside the chain where the look-ahead runs), the far block columns of L are kept transposed, and
every step of a sweep is one launch of row-split pieces.  The default from m = 4096 is the backward sweep alone (H); here
both sweeps are forced at small sizes with LPIPM_EXPERIMENTAL=1 LPIPM_SOLVE_COUPLED=1 (2 / 3: one of them alone) through
k_potrf + k_chol_solve; super-blocks are 512 wide at these sizes:

  m = 1000  padded to 1024, two super-blocks: near coupling only       m = 1536  three: the first far block
  m = 2048  four: the structure of the headline at width 512           m = 1400  1408 = 512 + 512 + 384: a partial last one
  m =  512  one super-block: the rule falls back to the plain sweep

Tolerances are those of tests/test_gpu_chain_bytes.py::test_solve_matches_oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [1000, 1536, 2048, 1400, 512]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.fixture(scope="module")
def coupled_env(built):
    """The knob is read when a factor plan is laid out (the first k_potrf of a size), so it stays set for the whole module."""
    mp = pytest.MonkeyPatch()
    mp.setenv("LPIPM_EXPERIMENTAL", "1")
    mp.setenv("LPIPM_SOLVE_COUPLED", "1")
    yield mp
    mp.undo()


@pytest.fixture(scope="module")
def contexts(coupled_env):
    """(forced look-ahead, serial schedule): the look-ahead knob is read when a context is created."""
    import lp_amd
    coupled_env.setenv("LPIPM_LOOKAHEAD", "1")
    ahead = lp_amd.Context(0)
    coupled_env.setenv("LPIPM_LOOKAHEAD", "0")
    serial = lp_amd.Context(0)
    coupled_env.delenv("LPIPM_LOOKAHEAD")
    yield ahead, serial
    ahead.close()
    serial.close()


@pytest.fixture(scope="module")
def cases(built):
    """Per shape: M, the oracle's factor, right-hand sides and the oracle's solutions, computed once."""
    from oracle import capi as oracle
    out = {}
    for m in SHAPES:
        rng = np.random.default_rng(m)
        B = rng.standard_normal((m, 2 * m + 3))
        M = B @ B.T + 1e-3 * np.eye(m)
        rc, Lref = oracle.cholesky(M)
        assert rc == 0
        R = rng.standard_normal((2, m))
        out[m] = (M, Lref, R, np.stack([oracle.cholesky_solve(Lref, R[q]) for q in range(2)]))
    return out


@pytest.mark.parametrize("m", SHAPES)
def test_coupled_solve_matches_oracle_and_is_schedule_independent(contexts, cases, m):
    ahead, serial = contexts
    M, Lref, R, Vref = cases[m]
    L, info, _ = ahead.k_potrf(M)
    assert info == 0
    assert np.abs(np.tril(L) - Lref).max() <= 1e-10 * np.abs(Lref).max()
    Ls, infos, _ = serial.k_potrf(M)
    assert infos == 0 and np.array_equal(np.tril(L), np.tril(Ls))
    nsb = -(-(-(-m // 128) * 128) // 512)
    for nrhs in (1, 2):
        V, _ = ahead.k_chol_solve(m, R[:nrhs])
        for q in range(nrhs):
            resid = np.abs(M @ V[q] - R[q]).max()
            print(f"[measure] m={m} nrhs={nrhs} q={q}: resid / (|M| |v|) {resid / (np.abs(M).sum(axis=1).max() * np.abs(V[q]).max()):.3g}, "
                  f"|v - v_oracle| / |v_oracle| {np.abs(V[q] - Vref[q]).max() / np.abs(Vref[q]).max():.3g}")
            assert resid <= 1e-12 * (np.abs(M).sum(axis=1).max() * np.abs(V[q]).max()), resid
            assert np.abs(V[q] - Vref[q]).max() <= 1e-9 * np.abs(Vref[q]).max()
        # the serial schedule (LPIPM_LOOKAHEAD=0) builds the same blocks in line: same bits
        Vs, _ = serial.k_chol_solve(m, R[:nrhs])
        assert _same(V, Vs)
        # ten solves on one context
        for _ in range(9):
            assert _same(ahead.k_chol_solve(m, R[:nrhs])[0], V)
        # the forward steps of the first super-blocks in a call of their own (SolveSteps), as the predictor runs them
        for split in sorted({0, 1, nsb - 1, nsb}):
            assert _same(ahead.k_chol_solve_split(m, R[:nrhs], split), V), split
    # a second factorisation on the same context rebuilds the same blocks
    L2, info2, _ = ahead.k_potrf(M)
    assert info2 == 0 and np.array_equal(np.tril(L2), np.tril(L))
    assert _same(ahead.k_chol_solve(m, R)[0], ahead.k_chol_solve_split(m, R, nsb - 1))


@pytest.mark.parametrize("m", [1000, 1536, 512])
def test_coupled_differs_from_plain_only_by_rounding(contexts, cases, coupled_env, m):
    """Against the plain sweep (knob at 0) on the same factor: equal for one super-block, rounding apart otherwise."""
    import lp_amd
    ahead, _ = contexts
    M, _, R, _ = cases[m]
    ahead.k_potrf(M)
    V, _ = ahead.k_chol_solve(m, R)
    coupled_env.setenv("LPIPM_SOLVE_COUPLED", "0")
    try:
        plain = lp_amd.Context(0)
        Lp, info, _ = plain.k_potrf(M)
        Vp, _ = plain.k_chol_solve(m, R)
        plain.close()
    finally:
        coupled_env.setenv("LPIPM_SOLVE_COUPLED", "1")
    assert info == 0
    if m == 512:
        assert _same(V, Vp)
    else:
        assert not _same(V, Vp)            # the knob took effect
        assert np.abs(V - Vp).max() <= 1e-9 * np.abs(Vp).max()


@pytest.mark.parametrize("m", [1536, 1400])
@pytest.mark.parametrize("part", ["2", "3"])
def test_each_sweep_coupled_alone(cases, coupled_env, part, m):
    """LPIPM_SOLVE_COUPLED=2: the backward sweep alone (the default from m = 4096), =3: the forward sweep alone; the other
    sweep is the plain one, and the two meet in the same vectors."""
    import lp_amd
    M, _, R, Vref = cases[m]
    coupled_env.setenv("LPIPM_SOLVE_COUPLED", part)
    try:
        ctx = lp_amd.Context(0)
        _, info, _ = ctx.k_potrf(M)
        V, _ = ctx.k_chol_solve(m, R)
        Vsplit = ctx.k_chol_solve_split(m, R, 2)
        ctx.close()
    finally:
        coupled_env.setenv("LPIPM_SOLVE_COUPLED", "1")
    assert info == 0 and _same(V, Vsplit)
    for q in range(2):
        assert np.abs(M @ V[q] - R[q]).max() <= 1e-12 * (np.abs(M).sum(axis=1).max() * np.abs(V[q]).max())
        assert np.abs(V[q] - Vref[q]).max() <= 1e-9 * np.abs(Vref[q]).max()


@pytest.mark.parametrize("m,k", [(1536, 0), (1536, 700), (1400, 1399), (2048, 1024)])
def test_nonpositive_pivot_reports_the_parents_info(contexts, cases, m, k):
    ahead, _ = contexts
    M, Lref, _, _ = cases[m]
    Mk = M.copy()
    Mk[k, k] -= 2.0 * Lref[k, k] ** 2
    _, info, _ = ahead.k_potrf(Mk)
    assert info == k + 1, info


def test_headline_solve_coupled_against_plain(built):
    """4096 x 8192 (tests/golden/planted_4096x8192_s0.npz is this LP's oracle record): the default (coupled) solve against
    the plain sweep: status 0, the same iteration count, x within the X_TOL of tests/test_gpu_solve.py."""
    import os
    import lp_amd
    from lp_amd import synth
    X_TOL = 1e-6
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planted_4096x8192_s0.npz"))
    A, b, c, _ = synth.planted_lp(0, 4096, 8192)
    opts = lp_amd.InteriorPoint.default().opts()
    mp = pytest.MonkeyPatch()
    try:
        mp.delenv("LPIPM_EXPERIMENTAL", raising=False)
        ctx = lp_amd.Context(0)
        ctx.upload_arrays(A, b, c)
        rc1, x1, _, it1, _ = ctx.solve_raw(opts)
        ctx.close()
        mp.setenv("LPIPM_EXPERIMENTAL", "1")
        mp.setenv("LPIPM_SOLVE_COUPLED", "0")
        ctx = lp_amd.Context(0)
        ctx.upload_arrays(A, b, c)
        rc0, x0, _, it0, _ = ctx.solve_raw(opts)
        ctx.close()
    finally:
        mp.undo()
    print(f"[measure] headline: iterations {it1} / {it0}, max|x_coupled - x_plain| {np.abs(x1 - x0).max():.3g}, "
          f"max|x_coupled - x_oracle| {np.abs(x1 - g['x_slack']).max():.3g}")
    assert rc1 == 0 and rc0 == 0
    assert it1 == it0
    assert np.abs(x1 - x0).max() <= X_TOL
    assert not _same(x1, x0)               # the default at this shape is the coupled sweep
