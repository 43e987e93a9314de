"""The factorisation's chain kernels load only what is read (lower triangle of the diagonal block, the triangle of
inv(L_kk) in the panel solve, whose products with its zeros are not run either) and skip band tiles nothing reads.
Every element keeps its k-ordered sum, so the factor, the 128-block inverses and both copies of the super-block inverses
must be, bit for bit up to the sign of an exact zero, what the commit before the change produced: their sha256 (of
X + 0.0, which folds -0.0 into +0.0) was recorded there into tests/golden/chain_bytes_parent.json by running this file as
a script against that build (python tests/test_gpu_chain_bytes.py --record FILE with its lp_amd first on PYTHONPATH).

Shapes, the smallest at which each path can go wrong: 128 (one block), 256, 384 (inside one outer panel: panel solve,
inner band updates with tiles above the diagonal skipped), 640 (second outer panel: one K = 512 update), 1000 (padded to
1024), 1536 with the look-ahead forced (the chain's K = 512 band, with its skipped tiles, and the side stream's
rest-update both run)."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_bytes_parent.json")
SHAPES = [(128, False), (256, False), (384, False), (640, False), (1000, False), (1536, True)]
PIVOTS = [5, 300]          # a non-positive pivot in block 0 and in the last block of m = 384
FORCE_ENV = {"LPIPM_EXPERIMENTAL": "1", "LPIPM_LOOKAHEAD": "1"}


def _matrix(m, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((m, m + 9))
    return B @ B.T


def _sha(X):
    return hashlib.sha256((np.ascontiguousarray(X) + 0.0).tobytes()).hexdigest()


def _blocks(X):
    n = X.shape[0] // 128
    return np.stack([X[k * 128:(k + 1) * 128, k * 128:(k + 1) * 128] for k in range(n)])


def _factor_hashes(ctx, m):
    L, info, _ = ctx.k_potrf(_matrix(m, 1000 + m))
    inv, invT, w = ctx.k_factor_inverses(m)
    return {"info": int(info), "super_w": int(w), "L": _sha(np.tril(L)), "blk_inv": _sha(_blocks(inv)),
            "blk_invT": _sha(_blocks(invT)), "sb_inv": _sha(inv), "sb_invT": _sha(invT)}


def _pivot_matrix(at):
    M = _matrix(384, 77)
    M[at, at] = -1.0
    return M


def _record(path):
    import lp_amd
    out = {"factor": {}, "pivot_info": {}}
    for m, force in SHAPES:
        saved = {k: os.environ.get(k) for k in FORCE_ENV}
        if force:
            os.environ.update(FORCE_ENV)
        ctx = lp_amd.Context(0)
        out["factor"][str(m)] = _factor_hashes(ctx, m)
        ctx.close()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    ctx = lp_amd.Context(0)
    for at in PIVOTS:
        out["pivot_info"][str(at)] = int(ctx.k_potrf(_pivot_matrix(at))[1])
    ctx.close()
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("m,force", SHAPES)
def test_factor_and_inverses_match_parent_bits(built, monkeypatch, golden, m, force):
    import lp_amd
    if force:
        for k, v in FORCE_ENV.items():
            monkeypatch.setenv(k, v)
    ctx = lp_amd.Context(0)
    got = _factor_hashes(ctx, m)
    ctx.close()
    assert got == golden["factor"][str(m)]


def test_lockstep_members_match_single_factor(ctx):
    """3 members at m = 384 factored as one lockstep batch: each factor is its single-LP factor bit for bit."""
    Ms = np.stack([_matrix(384, 40 + q) for q in range(3)])
    Ls, infos = ctx.k_potrf_lockstep(Ms)
    assert not infos.any()
    for q in range(3):
        L, info, _ = ctx.k_potrf(Ms[q])
        assert info == 0
        assert np.array_equal(np.tril(Ls[q]) + 0.0, np.tril(L) + 0.0)


@pytest.mark.parametrize("at", PIVOTS)
def test_nonpositive_pivot_info_matches_parent(ctx, golden, at):
    """After a failed pivot NaNs spread through fewer entries than before (the panel solve skips products with the zeros
    of inv(L_kk)); the info word is the parent's: 1 + the index of the first non-positive pivot."""
    _, info, _ = ctx.k_potrf(_pivot_matrix(at))
    assert info == golden["pivot_info"][str(at)] == at + 1


@pytest.mark.parametrize("m", [640, 1000])
def test_solve_matches_oracle(ctx, m):
    """k_potrf + k_chol_solve against the oracle's substitution, with the tolerances of test_potrf_and_solve."""
    from oracle import capi as oracle
    rng = np.random.default_rng(m)
    B = rng.standard_normal((m, 2 * m + 3))
    M = B @ B.T + 1e-3 * np.eye(m)
    L, info, _ = ctx.k_potrf(M)
    assert info == 0
    rc, Lref = oracle.cholesky(M)
    assert rc == 0
    assert np.abs(np.tril(L) - Lref).max() <= 1e-10 * np.abs(Lref).max()
    for nrhs in (1, 2):
        R = rng.standard_normal((nrhs, m))
        V, _ = ctx.k_chol_solve(m, R)
        for q in range(nrhs):
            resid = np.abs(M @ V[q] - R[q]).max()
            assert resid <= 1e-12 * (np.abs(M).sum(axis=1).max() * np.abs(V[q]).max()), resid
            vref = oracle.cholesky_solve(Lref, R[q])
            assert np.abs(V[q] - vref).max() <= 1e-9 * np.abs(vref).max()


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    _record(sys.argv[2])
