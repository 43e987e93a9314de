"""The work that runs beside the factorisation's chain on the look-ahead's side stream: the predictor's pass
A.W, the merges of the super-block inverses panel by panel, and the first forward steps of the predictor's solve.  Every
kernel runs with the arguments and on the data of the serial schedule; only the stream and the time differ.  So a solve
with the default schedule must equal, bit for bit, the solve of a fresh context under LPIPM_EXPERIMENTAL=1
LPIPM_LOOKAHEAD=0 (one stream, the serial order)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _solve(ctx, A, b, c):
    import lp_amd
    ctx.upload_arrays(A, b, c)
    rc, x, fun, it, rows = ctx.solve_raw(lp_amd.InteriorPoint.default().opts(), want_log=True)
    return rc, x, it, np.array(rows, dtype=np.float64)


def _same(a, b):
    # bit for bit, NaN included: compare the representations
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _serial_context(monkeypatch):
    import lp_amd
    monkeypatch.setenv("LPIPM_EXPERIMENTAL", "1")
    monkeypatch.setenv("LPIPM_LOOKAHEAD", "0")
    return lp_amd.Context(0)


def _default_context(monkeypatch, force):
    import lp_amd
    if force:
        monkeypatch.setenv("LPIPM_EXPERIMENTAL", "1")
        monkeypatch.setenv("LPIPM_LOOKAHEAD", "1")
    else:
        monkeypatch.delenv("LPIPM_LOOKAHEAD", raising=False)
        monkeypatch.delenv("LPIPM_EXPERIMENTAL", raising=False)
    return lp_amd.Context(0)


# the headline; the look-ahead forced below its threshold; mp / 128 = 36 (a partial last super-block, a short last outer
# panel); the smallest shape the path accepts
@pytest.mark.parametrize("m,n,force", [(4096, 8192, False), (2048, 4096, True), (4500, 6000, False), (1536, 3072, True)])
def test_solve_equals_the_serial_schedule(built, monkeypatch, m, n, force):
    from lp_amd import synth
    A, b, c, _ = synth.planted_lp(0, m, n)
    serial = _serial_context(monkeypatch)
    rc0, x0, it0, log0 = _solve(serial, A, b, c)
    serial.close()
    beside = _default_context(monkeypatch, force)
    rc1, x1, it1, log1 = _solve(beside, A, b, c)
    beside.close()
    assert rc0 == rc1 and it0 == it1 and it0 > 0
    assert log0.shape == (it0, 7) and _same(log0, log1)          # all seven columns of every iteration
    assert np.array_equal(x0, x1) and _same(x0, x1)


def test_ten_solves_on_one_context_are_identical(built, monkeypatch):
    """A dependency missing between the two streams shows up as bits that change from solve to solve."""
    from lp_amd import synth
    A, b, c, _ = synth.planted_lp(0, 4096, 8192)
    ctx = _default_context(monkeypatch, False)
    rc0, x0, it0, log0 = _solve(ctx, A, b, c)
    for _ in range(9):
        rc, x, it, log = _solve(ctx, A, b, c)
        assert rc == rc0 and it == it0 and _same(log, log0) and np.array_equal(x, x0) and _same(x, x0)
    ctx.close()


@pytest.mark.parametrize("m", [1536, 2048, 4608])
def test_kernel_entry_points_equal_the_serial_schedule(built, monkeypatch, m):
    """k_potrf on its own returns with every super-block inverse enqueued and joined: k_chol_solve behind it gives the
    serial context's solution bit for bit (the factor too)."""
    rng = np.random.default_rng(23)
    B = rng.standard_normal((m, m + 9))
    M = B @ B.T
    R = rng.standard_normal((2, m))
    serial = _serial_context(monkeypatch)
    L0, info0, _ = serial.k_potrf(M)
    V0, _ = serial.k_chol_solve(m, R)
    serial.close()
    forced = _default_context(monkeypatch, True)
    for _ in range(3):
        L1, info1, _ = forced.k_potrf(M)
        V1, _ = forced.k_chol_solve(m, R)
        assert info0 == 0 and info1 == 0
        assert np.array_equal(np.tril(L0), np.tril(L1)) and _same(V0, V1)
    forced.close()
