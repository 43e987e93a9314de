"""The pipelined chain step of the single-LP factorisation: the panel solve L21 = A21 . inv(L_kk)^T runs inside the
diagonal block's launch, column block by column block, as the rows of inv(L_kk) are handed over (kernels_potrf.hip).  Every
element keeps the sum gemm_nt_rows32_k128_kernel gives it, so everything must equal, bit for bit up to the sign of an exact
zero (X + 0.0, as test_gpu_chain_bytes.py), what the same build computes with LPIPM_PANEL_PIPE=0: the two launches.

Sizes, the smallest at which each path can go wrong: 256 (one pipelined step, two panel workgroups), 384 (8 then 4 row
tiles), 416 (padded to 512: a panel workgroup of one real tile and one of padding), 640 (a K = 512 band behind a pipelined
step), 1536 with the look-ahead forced (the side stream is busy beside the pipelined launches)."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PIPE_TIMEOUT = 1 << 30          # info word: a panel workgroup gave up waiting (kernels_potrf.hip)
OFF = {"LPIPM_EXPERIMENTAL": "1", "LPIPM_PANEL_PIPE": "0"}
LOOKAHEAD = {"LPIPM_EXPERIMENTAL": "1", "LPIPM_LOOKAHEAD": "1"}


def _matrix(m, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((m, m + 9))
    return B @ B.T


def _blocks(X):
    n = X.shape[0] // 128
    return np.stack([X[k * 128:(k + 1) * 128, k * 128:(k + 1) * 128] for k in range(n)])


def _factor(ctx, M):
    m = M.shape[0]
    L, info, _ = ctx.k_potrf(M)
    inv, invT, w = ctx.k_factor_inverses(m)
    return {"info": np.int64(info), "super_w": np.int64(w), "L": np.tril(L) + 0.0, "blk_inv": _blocks(inv) + 0.0,
            "blk_invT": _blocks(invT) + 0.0, "sb_inv": inv + 0.0, "sb_invT": invT + 0.0}


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("m,force", [(256, False), (384, False), (416, False), (640, False), (1536, True)])
def test_factor_and_inverses_equal_two_launches(built, monkeypatch, m, force):
    import lp_amd
    if force:
        _setenv(monkeypatch, LOOKAHEAD)
    ctx = lp_amd.Context(0)                       # (the look-ahead is a property of the context, the pipe is read per call)
    M = _matrix(m, 2000 + m)
    on = _factor(ctx, M)
    _setenv(monkeypatch, OFF)
    off = _factor(ctx, M)
    ctx.close()
    assert on["info"] == 0 and off["info"] == 0
    for k in off:
        assert np.array_equal(on[k], off[k]), k


def test_flag_words_return_to_zero(ctx):
    """Fifty factorisations on one context: the hand-off words are cleared inside each launch, never by the host, so a word
    left raised would let a later panel workgroup read rows of the inverse that are not there yet."""
    M = _matrix(640, 31)
    seen = set()
    for _ in range(50):
        L, info, _ = ctx.k_potrf(M)
        assert info == 0
        seen.add(hashlib.sha256((np.tril(L) + 0.0).tobytes()).hexdigest())
    assert len(seen) == 1


@pytest.mark.parametrize("at", [5, 128 + 37, 300])
def test_nonpositive_pivot_does_not_strand_the_panel(ctx, monkeypatch, at):
    """A failed pivot in block 0, inside block 1 and in the last block of m = 384: the diagonal-block workgroup raises its
    flags all the same, the call returns without a time-out and reports what the two launches report."""
    M = _matrix(384, 77)
    M[at, at] = -1.0
    info_on = ctx.k_potrf(M)[1]
    _setenv(monkeypatch, OFF)
    info_off = ctx.k_potrf(M)[1]
    assert info_off == at + 1               # the reference path reports this failure
    assert not info_on & PIPE_TIMEOUT
    assert info_on == info_off
    monkeypatch.delenv("LPIPM_PANEL_PIPE")
    monkeypatch.delenv("LPIPM_EXPERIMENTAL")
    L, info, _ = ctx.k_potrf(_matrix(384, 78))   # and the next factorisation finds its flag words at zero
    _setenv(monkeypatch, OFF)
    L0, info0, _ = ctx.k_potrf(_matrix(384, 78))
    assert info == 0 and info0 == 0 and np.array_equal(np.tril(L) + 0.0, np.tril(L0) + 0.0)


@pytest.mark.parametrize("m,n", [(384, 768), (640, 1280)])
def test_whole_solve_equals_two_launches(ctx, monkeypatch, m, n):
    import lp_amd
    from lp_amd import synth
    A, b, c, _ = synth.planted_lp(3, m, n)
    o = lp_amd.InteriorPoint.default().opts()
    ctx.upload_arrays(A, b, c)
    rc, x, fun, it, _ = ctx.solve_raw(o)
    _setenv(monkeypatch, OFF)
    ctx.upload_arrays(A, b, c)
    rc0, x0, fun0, it0, _ = ctx.solve_raw(o)
    assert rc == rc0 == 0 and it == it0
    assert np.array_equal(x + 0.0, x0 + 0.0) and fun == fun0


def test_lockstep_batch_equals_members_alone(ctx):
    """The batch path is untouched (its diagonal-block launches stay one workgroup per member, followed by the panel launch);
    the members solved alone take the pipelined step."""
    import lp_amd
    from lp_amd import synth
    probs = [synth.planted_lp(s, 256, 512)[:3] for s in range(3)]
    o = lp_amd.InteriorPoint.default().opts()
    ctx.upload_lockstep([p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs])
    res = ctx.solve_lockstep(o)
    for (A, b, c), (status, x, fun, it) in zip(probs, res):
        ctx.upload_arrays(A, b, c)
        rc1, x1, fun1, it1, _ = ctx.solve_raw(o)
        assert status == rc1 == 0 and it == it1
        assert np.array_equal(x + 0.0, x1 + 0.0) and fun == fun1
