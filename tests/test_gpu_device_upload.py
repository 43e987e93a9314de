"""lpipm_upload_device: problems and batches made resident from strided DEVICE memory (torch CUDA tensors), DESIGN 3.11.

The yardstick is the host upload of the same numbers: an upload is a copy, so the resident image, every solve, every later
update and every byte count after lpipm_upload_device are those after the equivalent host entry, bit for bit.  Inputs are
lp_amd.synth's planted matrices and vectors.

1. the packed image (lpipm_k_resident_matrix) for every tile edge, padding step and source layout;
2. one solve through each host entry and through its descriptor;
3. the slack hint, verified on the device;
4. the context afterwards: new vectors, scaling, the kept first factor, a second upload into the same geometry;
5. the refusals, each made on the host before anything is enqueued;
6. lp_amd.batch.solve_device end to end."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MS = (1, 5, 31, 64, 65, 129, 200)          # rows: the tile edges 32 and 64, the 128-row padding step, a single row
NXS = (1, 3, 17, 33, 64, 100, 130)         # columns: the 16-column padding step, the 128-column tile of the row modes
INF = 1                                    # the member of every batch that is infeasible


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mat(seed, m, n):
    """An m x n matrix of synth.planted_lp's normals (the generator wants m <= n: a tall one is a transpose)."""
    from lp_amd import synth
    A = synth.planted_lp(seed, m, n)[0] if m <= n else synth.planted_lp(seed, n, m)[0].T.copy()
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def _vecs(seed, n):
    """x* in [1, 2)^n and a cost vector >= 0.1 (so that every feasible member is bounded), from the same generator."""
    from lp_amd import synth
    _, _, c, xs = synth.planted_lp(seed, n, n)
    c = np.abs(c) + 0.1
    c.setflags(write=False); xs.setflags(write=False)
    return xs, c


@functools.lru_cache(maxsize=None)
def _blocks(seed, m_ub, m_eq, n):
    """A_ub, A_eq of one inequality-form LP; row 0 is >= 0, so a right-hand side of -1 there makes a member infeasible."""
    G = _mat(seed, m_ub + m_eq, n).copy()
    G[0] = np.abs(G[0])
    G.setflags(write=False)
    return G[:m_ub], G[m_ub:]


@functools.lru_cache(maxsize=None)
def _member(seed, m_ub, m_eq, n, k, infeasible=False):
    """b = [b_ub; b_eq], c, c0 of member k over the blocks of `seed`."""
    A_ub, A_eq = _blocks(seed, m_ub, m_eq, n)
    xs, c = _vecs(1000 * seed + k, n)
    b = np.concatenate([A_ub @ xs + 1.0, A_eq @ xs])
    if infeasible:
        b[0] = -1.0
    b.setflags(write=False)
    return b, c, 0.25 * k


def _slack_form(A_ub, A_eq):
    m_ub, n = A_ub.shape
    S = np.zeros((m_ub + A_eq.shape[0], n + m_ub))
    S[:m_ub, :n], S[m_ub:, :n] = A_ub, A_eq
    S[np.arange(m_ub), n + np.arange(m_ub)] = 1.0
    return S


def _slack_cost(c, m_ub):
    return np.concatenate([c, np.zeros(m_ub)])


def T(a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a, order="C")).cuda()               # (a copy: the cached inputs are read-only)
    return t if dtype is None else t.to(dtype)


def _opts(**kw):
    import lp_amd
    o = lp_amd.InteriorPoint.default().opts()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _norm(rc, x, fun, it):
    """One result as comparable bit patterns (NaN-safe)."""
    has_x = rc in (0, 7)
    return int(rc), _bits(x).tobytes() if has_x else None, _bits(np.float64(fun)).tobytes() if has_x else None, int(it)


def _solve(cx, o, batch):
    if batch:
        return [_norm(*r) for r in cx.solve_lockstep(o)]
    return [_norm(*cx.solve_raw(o)[:4])]


def _both_solves(cx, batch):
    """The default solve, then one that stops at max_iter = 3: every exit is crossed."""
    return _solve(cx, _opts(), batch), _solve(cx, _opts(max_iter=3), batch)


@pytest.fixture(scope="module")
def pair(built):
    """(host, dev): two contexts of their own -- one takes the host uploads, the other the device uploads."""
    import lp_amd
    host, dev = lp_amd.Context(0), lp_amd.Context(0)
    yield host, dev
    host.close(); dev.close()


# ---- 1. the packed image, bit for bit -----------------------------------------------------------------------------------------------
def _layout(A, kind):
    """A torch CUDA view with A's values in the layout `kind`."""
    import torch
    m, nx = A.shape
    if kind == "contiguous":
        return T(A)
    if kind in ("pitch_odd_offset", "pitch_even_offset"):      # a leading dimension > n; 8-byte / 16-byte aligned base
        odd = kind == "pitch_odd_offset"
        pitch, off = (nx + 5, 1) if odd else (nx + nx % 2 + 6, 2)
        buf = torch.full((off + m * pitch + 3,), float("nan"), dtype=torch.float64, device="cuda")
        v = buf[off:off + m * pitch].view(m, pitch)[:, :nx]
        v.copy_(T(A))
        assert v.data_ptr() % 16 == (8 if odd else 0) and v.stride() == (pitch, 1)
        return v
    if kind == "column_major":
        v = T(A.T.copy()).t()
        assert v.shape == (m, nx) and (v.stride() == (1, m) or 1 in (m, nx))
        return v
    if kind == "strided":
        big = torch.full((2 * m, 3 * nx), float("nan"), dtype=torch.float64, device="cuda")
        v = big[::2, ::3]
        v.copy_(T(A))
        return v
    if kind == "f32":
        return T(A.astype(np.float32))
    if kind == "f32_column_major":
        return T(A.astype(np.float32).T.copy()).t()
    raise AssertionError(kind)


@functools.lru_cache(maxsize=None)
def _host_image(m, nx, f32):
    """The image the host upload of the m x nx matrix leaves (of its float32 rounding, widened, when f32): computed once."""
    import lp_amd
    A = _mat(11, m, nx)
    A = A.astype(np.float32).astype(np.float64) if f32 else A
    cx = lp_amd.Context(0)
    cx.upload_arrays(A, np.ones(m), np.ones(nx))
    img = cx.k_resident_matrix(0)
    cx.close()
    img.setflags(write=False)
    return img


LAYOUTS = ("contiguous", "pitch_odd_offset", "pitch_even_offset", "column_major", "strided", "f32", "f32_column_major")


@pytest.mark.parametrize("kind", LAYOUTS)
def test_image_of_a_single_lp(pair, kind):
    import torch
    _, dev = pair
    f32 = kind.startswith("f32")
    dt = torch.float32 if f32 else torch.float64
    for m in MS:
        for nx in NXS:
            A = _mat(11, m, nx)
            want = _host_image(m, nx, f32)
            dev.upload_device(_layout(A, kind), torch.ones(m, dtype=dt, device="cuda"), torch.ones(nx, dtype=dt, device="cuda"))
            got = dev.k_resident_matrix(0)
            assert got.shape == want.shape == (-(-m // 128) * 128, -(-nx // 16) * 16)
            assert np.array_equal(_bits(got), _bits(want)), (kind, m, nx)


@pytest.mark.parametrize("kind", ["row_major", "column_major"])
def test_image_of_members_cut_out_of_one_tensor(pair, kind):
    """Members 0, 2, 4 of a [5, m, n] tensor: the member stride is twice a member."""
    import torch
    host, dev = pair
    for m in MS:
        for nx in NXS:
            As = [_mat(20 + k, m, nx) for k in range(5)]
            big = T(np.stack(As)) if kind == "row_major" else T(np.stack([A.T for A in As])).transpose(1, 2)
            view = big[::2]
            assert view.shape == (3, m, nx) and (view.stride(0) == 2 * m * nx)
            ones = lambda n: torch.ones(3, n, dtype=torch.float64, device="cuda")
            host.upload_lockstep(As[::2], [np.ones(m)] * 3, [np.ones(nx)] * 3)
            dev.upload_device(view, ones(m), ones(nx))
            for k in range(3):
                assert np.array_equal(_bits(dev.k_resident_matrix(k)), _bits(host.k_resident_matrix(k))), (kind, m, nx, k)
            assert dev.resident_bytes() == host.resident_bytes()


@pytest.mark.parametrize("m_ub,m_eq", [(0, 7), (7, 0), (33, 31)])
@pytest.mark.parametrize("kinds", [("contiguous", "column_major"), ("column_major", "pitch_odd_offset"), ("f32", "f32_column_major")])
def test_image_of_ub_and_eq_blocks(pair, m_ub, m_eq, kinds):
    """The two blocks of rows of the UB_EQ form, each in a layout of its own, at row offsets 0 and m_ub."""
    import torch
    import lp_amd
    host, dev = pair
    n = 17
    f32 = kinds[0].startswith("f32")
    rnd = (lambda a: a.astype(np.float32).astype(np.float64)) if f32 else (lambda a: a)
    A_ub, A_eq = _blocks(31, m_ub, m_eq, n)
    b, c, _ = _member(31, m_ub, m_eq, n, 0)
    pb = lp_amd.Problem.target(rnd(c))
    if m_ub:
        pb = pb.ub(rnd(A_ub), rnd(b[:m_ub]))
    if m_eq:
        pb = pb.eq(rnd(A_eq), rnd(b[m_ub:]))
    host.upload(pb.build())
    dt = torch.float32 if f32 else torch.float64
    A_t = _layout(A_ub, kinds[0]) if m_ub else torch.empty((0, n), dtype=dt, device="cuda")
    dev.upload_device(A_t, T(b, dt), T(c, dt), form="ub_eq", A_eq=_layout(A_eq, kinds[1]) if m_eq else None)
    assert (dev.m, dev.n) == (host.m, host.n) == (m_ub + m_eq, n + m_ub)
    assert np.array_equal(_bits(dev.k_resident_matrix(0)), _bits(host.k_resident_matrix(0)))
    assert dev.resident_bytes() == host.resident_bytes()
    assert _both_solves(dev, False) == _both_solves(host, False)


# ---- 2. solves, bit for bit: every host entry and its descriptor ---------------------------------------------------------------------
SL = (24, 16, 76)            # slack-form members: 24 ub + 16 eq rows, 76 structural columns -> 40 x 100 with 24 slack columns
UE = (30, 10, 60)            # ub / eq members
TL = (150, 0, 12)            # tall members


def _members(shape, seed, K):
    return [_member(seed, *shape, k, infeasible=(k == INF)) for k in range(K)]


def _case_single_slack(host, dev, n_slack):
    A_ub, A_eq = _blocks(41, *SL)
    b, c, c0 = _member(41, *SL, 2)
    S, cs = _slack_form(A_ub, A_eq), _slack_cost(c, SL[0])
    host.upload_arrays(S, b, cs, c0, n_slack)
    dev.upload_device(T(S), T(b), T(cs), [c0], n_slack=n_slack)
    return False


def _case_ub_eq(host, dev):
    import lp_amd
    A_ub, A_eq = _blocks(42, *UE)
    b, c, _ = _member(42, *UE, 0)
    host.upload(lp_amd.Problem.target(c).ub(A_ub, b[:UE[0]]).eq(A_eq, b[UE[0]:]).build())
    dev.upload_device(T(A_ub), T(b), T(c), form="ub_eq", A_eq=T(A_eq.T.copy()).t())
    return False


def _case_ub_tall(host, dev):
    import lp_amd
    A_ub, _ = _blocks(43, *TL)
    b, c, _ = _member(43, *TL, 0)
    host.upload(lp_amd.Problem.target(c).ub(A_ub, b).build(), tall=True)
    dev.upload_device(T(A_ub.T.copy()).t(), T(b), T(c), form="ub_tall")
    return False


def _case_lockstep(host, dev, K, n_slack):
    mats = [_slack_form(*_blocks(50 + k, *SL)) for k in range(K)]
    mem = [_member(50 + k, *SL, k, infeasible=(k == INF)) for k in range(K)]
    bs, cs, c0s = [m[0] for m in mem], [_slack_cost(m[1], SL[0]) for m in mem], [m[2] for m in mem]
    host.upload_lockstep(mats, bs, cs, c0s, n_slack=n_slack)
    dev.upload_device(T(np.stack(mats)), T(np.stack(bs)), T(np.stack(cs)), c0s, n_slack=n_slack)
    return True


def _case_shared(host, dev, K, n_slack):
    S = _slack_form(*_blocks(44, *SL))
    mem = _members(SL, 44, K)
    bs, cs, c0s = [m[0] for m in mem], [_slack_cost(m[1], SL[0]) for m in mem], [m[2] for m in mem]
    host.upload_lockstep_shared(S, bs, cs, c0s, n_slack=n_slack)
    dev.upload_device(T(S), T(np.stack(bs)), T(np.stack(cs)), c0s, n_slack=n_slack)
    return True


def _case_shared_ub_eq(host, dev, K):
    A_ub, A_eq = _blocks(45, *UE)
    mem = _members(UE, 45, K)
    bs, cs, c0s = [m[0] for m in mem], [m[1] for m in mem], [m[2] for m in mem]
    host.upload_lockstep_shared_ub_eq(A_ub, A_eq, bs, cs, c0s)
    dev.upload_device(T(A_ub), T(np.stack(bs)), T(np.stack(cs)), c0s, form="ub_eq", A_eq=T(A_eq))
    return True


def _case_shared_ub_tall(host, dev, K):
    A_ub, _ = _blocks(46, *TL)
    mem = _members(TL, 46, K)
    bs, cs, c0s = [m[0] for m in mem], [m[1] for m in mem], [m[2] for m in mem]
    host.upload_lockstep_shared_ub_tall(A_ub, bs, cs, c0s)
    dev.upload_device(T(A_ub), T(np.stack(bs)), T(np.stack(cs)), c0s, form="ub_tall")
    return True


def _case_lockstep_ub_tall(host, dev, K):
    mats = [_blocks(60 + k, *TL)[0] for k in range(K)]
    mem = [_member(60 + k, *TL, k, infeasible=(k == INF)) for k in range(K)]
    bs, cs, c0s = [m[0] for m in mem], [m[1] for m in mem], [m[2] for m in mem]
    host.upload_lockstep_ub_tall(mats, bs, cs, c0s)
    dev.upload_device(T(np.stack(mats)), T(np.stack(bs)), T(np.stack(cs)), c0s, form="ub_tall")
    return True


CASES = {
    "lpipm_upload": lambda h, d: _case_single_slack(h, d, 0),
    "lpipm_upload_slack": lambda h, d: _case_single_slack(h, d, 24),
    "lpipm_upload_ub_eq": _case_ub_eq,
    "lpipm_upload_ub_tall": _case_ub_tall,
    "lpipm_upload_lockstep": lambda h, d: _case_lockstep(h, d, 3, 0),
    "lpipm_upload_lockstep_slack": lambda h, d: _case_lockstep(h, d, 5, 24),
    "lpipm_upload_lockstep_shared": lambda h, d: _case_shared(h, d, 3, 0),
    "lpipm_upload_lockstep_shared_slack": lambda h, d: _case_shared(h, d, 5, 24),
    "lpipm_upload_lockstep_shared_ub_eq": lambda h, d: _case_shared_ub_eq(h, d, 3),
    "lpipm_upload_lockstep_shared_ub_tall": lambda h, d: _case_shared_ub_tall(h, d, 5),
    "lpipm_upload_lockstep_ub_tall": lambda h, d: _case_lockstep_ub_tall(h, d, 3),
}


@pytest.mark.parametrize("entry", list(CASES))
def test_solve_equals_the_host_entry(pair, entry):
    host, dev = pair
    batch = CASES[entry](host, dev)
    assert (dev.m, dev.n) == (host.m, host.n)
    assert dev.resident_bytes() == host.resident_bytes()
    want, got = _both_solves(host, batch), _both_solves(dev, batch)
    assert got == want
    assert all(r[0] == 7 for r in want[1])                            # max_iter = 3 stops every member ...
    if batch:
        assert want[0][INF][0] == 5 and want[0][0][0] == 0           # ... and the default solve has both other exits


# ---- 3. the hint on the device -------------------------------------------------------------------------------------------------------
def _hint_batch(disturb=None):
    """Three slack-form members (40 x 100, 24 slack columns); `disturb` changes one entry of the last member's slack block."""
    mats = [_slack_form(*_blocks(70 + k, *SL)) for k in range(3)]
    if disturb is not None:
        i, j, v = disturb
        mats[2][i, SL[2] + j] = v
    mem = [_member(70 + k, *SL, k) for k in range(3)]
    return mats, [m[0] for m in mem], [_slack_cost(m[1], SL[0]) for m in mem]


DISTURBED = {"diagonal_one_ulp": (5, 5, np.nextafter(1.0, 2.0)), "off_diagonal_denormal": (30, 2, 5e-324), "nan": (3, 9, np.nan)}


def test_a_true_hint_is_used(pair):
    host, dev = pair
    mats, bs, cs = _hint_batch()
    host.upload_lockstep(mats, bs, cs)
    dense = host.resident_bytes()
    host.upload_lockstep(mats, bs, cs, n_slack=24)
    dev.upload_device(T(np.stack(mats)), T(np.stack(bs)), T(np.stack(cs)), n_slack=24)
    assert dev.resident_bytes() == host.resident_bytes() < dense
    assert np.array_equal(_bits(dev.k_resident_matrix(2)), _bits(host.k_resident_matrix(2)))
    assert dev.k_resident_matrix(2).shape == (128, 80)               # the 76 structural columns only
    assert _solve(dev, _opts(), True) == _solve(host, _opts(), True)


@pytest.mark.parametrize("what", list(DISTURBED))
@pytest.mark.parametrize("layout", ["row_major", "column_major"])
def test_a_disturbed_hint_gives_the_dense_upload(pair, what, layout):
    host, dev = pair
    clean = _hint_batch()
    host.upload_lockstep(*clean)
    dense = host.resident_bytes()
    mats, bs, cs = _hint_batch(DISTURBED[what])
    host.upload_lockstep(mats, bs, cs, n_slack=24)
    A = T(np.stack(mats)) if layout == "row_major" else T(np.stack([M.T for M in mats])).transpose(1, 2)
    dev.upload_device(A, T(np.stack(bs)), T(np.stack(cs)), n_slack=24)
    assert dev.resident_bytes() == host.resident_bytes() == dense
    assert _solve(dev, _opts(), True) == _solve(host, _opts(), True)


def test_a_hint_of_all_columns_is_ignored(pair):
    host, dev = pair
    S = np.zeros((40, 24)); S[np.arange(24), np.arange(24)] = 1.0
    b, c = np.concatenate([np.ones(24), np.zeros(16)]), np.ones(24)
    host.upload_arrays(S, b, c, 0.0, 24)
    dev.upload_device(T(S), T(b), T(c), n_slack=24)
    assert dev.resident_bytes() == host.resident_bytes()
    assert np.array_equal(_bits(dev.k_resident_matrix(0)), _bits(host.k_resident_matrix(0)))
    assert _solve(dev, _opts(), False) == _solve(host, _opts(), False)


@pytest.mark.parametrize("what", [None, "diagonal_one_ulp"])
def test_a_shared_batch_checks_its_one_matrix(pair, what):
    host, dev = pair
    S = _slack_form(*_blocks(44, *SL))
    if what:
        i, j, v = DISTURBED[what]
        S[i, SL[2] + j] = v
    mem = _members(SL, 44, 3)
    bs, cs = [m[0] for m in mem], [_slack_cost(m[1], SL[0]) for m in mem]
    host.upload_lockstep_shared(S, bs, cs)
    dense = host.resident_bytes()
    host.upload_lockstep_shared(S, bs, cs, n_slack=24)
    dev.upload_device(T(S), T(np.stack(bs)), T(np.stack(cs)), n_slack=24)
    assert dev.resident_bytes() == host.resident_bytes()
    assert (host.resident_bytes() == dense) == bool(what)
    assert _solve(dev, _opts(), True) == _solve(host, _opts(), True)


# ---- 4. the context afterwards is the host upload's ----------------------------------------------------------------------------------
def test_new_vectors_for_a_batch(pair):
    host, dev = pair
    _case_lockstep(host, dev, 3, 24)
    new = [_member(80 + k, *SL, k) for k in range(3)]
    mats = [_slack_form(*_blocks(50 + k, *SL)) for k in range(3)]
    xs = [_vecs(900 + k, SL[2] + SL[0])[0] for k in range(3)]
    bs = [mats[k] @ xs[k] for k in range(3)]                          # feasible for member k's own matrix
    cs, c0s = [_slack_cost(m[1], SL[0]) for m in new], [1.0, 2.0, 3.0]
    for cx in (host, dev):
        cx.update_lockstep_vectors(bs, cs, c0s)
    assert _both_solves(dev, True) == _both_solves(host, True)
    bt, ct = T(np.stack(bs[::-1])), T(np.stack(cs[::-1]))
    import torch
    torch.cuda.synchronize()
    for cx in (host, dev):
        cx.update_lockstep_vectors_device(bt.data_ptr(), bt.stride(0), ct.data_ptr(), ct.stride(0), c0s[::-1])
    assert _both_solves(dev, True) == _both_solves(host, True)


def test_update_vectors_device_equals_update_vectors(pair):
    host, dev = pair
    _case_single_slack(host, dev, 24)
    S = _slack_form(*_blocks(41, *SL))
    b = S @ _vecs(901, SL[2] + SL[0])[0]
    c = _slack_cost(_vecs(902, SL[2])[1], SL[0])
    host.update_vectors(b, c)
    dev.update_vectors_device(T(b), T(c))
    want = _both_solves(host, False)
    assert _both_solves(dev, False) == want and want[0][0][0] == 0
    dev.update_vectors(b[::-1].copy(), c)                             # and the host entry works after a device upload
    host.update_vectors_device(T(b[::-1].copy()), T(c))
    assert _both_solves(dev, False) == _both_solves(host, False)


def test_scaling_after_a_device_upload(built):
    import lp_amd
    host, dev = lp_amd.Context(0), lp_amd.Context(0)
    mats = [_slack_form(*_blocks(50 + k, *SL)).copy() for k in range(3)]
    for k, M in enumerate(mats):                                       # rows and columns of mixed units: 2^+-16
        M[3 + k, :SL[2]] *= 2.0 ** 16
        M[:, 7 + k] *= 2.0 ** -16
        M[20, :SL[2]] *= 2.0 ** -16
    mem = [_member(50 + k, *SL, k) for k in range(3)]
    xs = [_vecs(910 + k, SL[2] + SL[0])[0] for k in range(3)]
    bs, cs = [mats[k] @ xs[k] for k in range(3)], [_slack_cost(m[1], SL[0]) for m in mem]
    for cx in (host, dev):
        cx.set_scaling(8)
    host.upload_lockstep(mats, bs, cs, n_slack=24)
    dev.upload_device(T(np.stack(mats)), T(np.stack(bs)), T(np.stack(cs)), n_slack=24)
    assert dev.resident_bytes() == host.resident_bytes()
    for k in range(3):
        (kr_h, kc_h), (kr_d, kc_d) = host.scaling(k), dev.scaling(k)
        assert np.array_equal(kr_h, kr_d) and np.array_equal(kc_h, kc_d)
        assert np.abs(kr_h).max() >= 4                               # the exponents are not trivially zero
        assert np.array_equal(_bits(dev.k_resident_matrix(k)), _bits(host.k_resident_matrix(k)))
    assert _both_solves(dev, True) == _both_solves(host, True)
    host.close(); dev.close()


def test_the_first_factor_is_kept_after_a_device_upload(built):
    import lp_amd
    A_ub, A_eq = _blocks(41, *SL)
    b, c, c0 = _member(41, *SL, 2)
    S, cs = _slack_form(A_ub, A_eq), _slack_cost(c, SL[0])
    seen = {}
    for name in ("host", "device"):
        cx = lp_amd.Context(0)
        cx.set_profiling(2)
        if name == "host":
            cx.upload_arrays(S, b, cs, c0, 24)
        else:
            cx.upload_device(T(S), T(b), T(cs), [c0], n_slack=24)
        runs = []
        for _ in range(2):
            r = _norm(*cx.solve_raw(_opts())[:4])
            runs.append((r, cx.phase_times()["adat_launches"], cx.phase_times()["iterations"]))
        seen[name] = runs
        cx.close()
    assert seen["device"] == seen["host"]
    (r1, launches1, its1), (r2, launches2, its2) = seen["device"]
    assert r1 == r2 and r1[0] == 0 and launches1 == its1 and launches2 == its2 - 1


def test_a_second_upload_into_the_same_geometry_leaves_nothing_stale(built):
    """m = 60, then m = 50 with n unchanged: one padded geometry, so the second upload reuses the allocations of the first."""
    import lp_amd
    n = 90
    reused, fresh = lp_amd.Context(0), lp_amd.Context(0)
    def up(cx, m, seed):
        A = _mat(seed, m, n)
        xs, c = _vecs(seed, n)
        cx.upload_device(T(A), T(A @ xs), T(c))
    up(reused, 60, 95)
    first = reused.resident_bytes()
    up(reused, 50, 96)
    up(fresh, 50, 96)
    assert reused.resident_bytes() == fresh.resident_bytes() == first
    img = reused.k_resident_matrix(0)
    assert np.array_equal(_bits(img), _bits(fresh.k_resident_matrix(0))) and not img[50:].any() and not img[:, n:].any()
    assert _both_solves(reused, False) == _both_solves(fresh, False)
    reused.close(); fresh.close()


def test_the_timed_pack_launch_rewrites_the_image_it_found(pair):
    """lpipm_k_pack_matrix (the measuring hook of profiles/device_upload.md) runs the upload's own launch again."""
    import lp_amd
    _, dev = pair
    mats = [_blocks(60 + k, *TL)[0] for k in range(3)]
    A, b, c = T(np.stack([M.T for M in mats])).transpose(1, 2), T(np.ones((3, TL[0]))), T(np.ones((3, TL[2])))
    dev.upload_device(A, b, c, form="ub_tall")
    before = [dev.k_resident_matrix(k) for k in range(3)]
    pack_ms, copy_ms = dev.k_pack_matrix(A, b, c, repeats=2, form="ub_tall")
    assert pack_ms > 0.0 and copy_ms > 0.0
    assert all(np.array_equal(_bits(dev.k_resident_matrix(k)), _bits(before[k])) for k in range(3))
    with pytest.raises(lp_amd.BackendError):                           # another shape than the resident one
        dev.k_pack_matrix(A[:2], b[:2], c[:2], repeats=1, form="ub_tall")
    assert all(np.array_equal(_bits(dev.k_resident_matrix(k)), _bits(before[k])) for k in range(3))


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
class _Collective:
    def __init__(self):
        from lp_amd import _capi
        self.cfn = _capi.ALLREDUCE_FN(lambda *a: 1)


def _descriptor(A, b, c, **kw):
    import lp_amd
    return lp_amd._device_request(A, b, c, **kw)[:2]


def test_refusals_leave_the_resident_problem_alone(built):
    import torch
    import lp_amd
    from lp_amd import _capi
    L = _capi.lib()
    cx = lp_amd.Context(0)
    b0, c0, k0 = _member(41, *SL, 2)
    cx.upload_device(T(_slack_form(*_blocks(41, *SL))), T(b0), T(_slack_cost(c0, SL[0])), [k0], n_slack=24)
    before = _solve(cx, _opts(), False)
    bytes_before = cx.resident_bytes()
    m, n = 40, 100
    A, b, c = T(_mat(97, m, n)), T(np.ones(m)), T(np.ones(n))
    hA, hb, hc = np.ones((m, n)), np.ones(m), np.ones(n)
    hp = lambda a: a.ctypes.data

    def refused(want, change, **kw):
        d, keep = _descriptor(kw.pop("A", A), kw.pop("b", b), kw.pop("c", c), **kw)
        change(d)
        torch.cuda.synchronize()
        assert L.lpipm_upload_device(cx._h, C.byref(d)) == want
        assert cx.resident_bytes() == bytes_before and _solve(cx, _opts(), False) == before

    bad, unsupported = _capi.ERR_BAD_ARGUMENT, _capi.ERR_UNSUPPORTED
    probe = lp_amd.Context(0)                                          # (the descriptor these cases start from is a good one)
    good, keep = _descriptor(A, b, c)
    assert L.lpipm_upload_device(probe._h, C.byref(good)) == _capi.OK
    probe.close()
    refused(bad, lambda d: setattr(d.A, "ptr", hp(hA)))               # host (numpy) memory in each place
    refused(bad, lambda d: setattr(d.b, "ptr", hp(hb)))
    refused(bad, lambda d: setattr(d.c, "ptr", hp(hc)))
    refused(bad, lambda d: setattr(d, "m", 1 << 40))                   # extents far beyond the tensor
    refused(bad, lambda d: (setattr(d, "m", 1 << 20), setattr(d, "n", 4096)))      # ... within the limits on m and n: ~0.8 GB
    refused(bad, lambda d: setattr(d.A, "row_stride", 1 << 40))       # ... and through a stride
    refused(bad, lambda d: setattr(d.A, "row_stride", 0))
    refused(bad, lambda d: setattr(d.c, "stride", 0))
    refused(bad, lambda d: setattr(d, "struct_size", d.struct_size - 8))
    refused(bad, lambda d: setattr(d, "count", 0))
    refused(bad, lambda d: setattr(d, "count", 4097))
    refused(bad, lambda d: setattr(d, "form", 3))
    refused(bad, lambda d: setattr(d, "src_type", 2))
    refused(_capi.UNCONSTRAINED, lambda d: setattr(d, "m", 0))
    refused(bad, lambda d: setattr(d, "n", 0))
    refused(bad, lambda d: setattr(d, "n_slack", n + 1))
    refused(bad, lambda d: setattr(d, "n_slack", m + 1))
    refused(bad, lambda d: setattr(d.A, "ptr", None))
    A3 = T(np.stack([_mat(98 + k, 8, 12) for k in range(3)]))
    refused(unsupported, lambda d: None, A=A3, b=T(np.ones((3, 10))), c=T(np.ones((3, 12))), form="ub_eq", A_eq=T(np.ones((2, 12))))
    # the last member of a batch reaches beyond the tensor the batch was cut from
    refused(bad, lambda d: setattr(d.A, "member_stride", 1 << 30), A=A3, b=T(np.ones((3, 8))), c=T(np.ones((3, 12))))
    # the same calls through the method raise and change nothing
    with pytest.raises(lp_amd.BackendError):
        cx.upload_device(A3, T(np.ones((3, 10))), T(np.ones((3, 12))), form="ub_eq", A_eq=T(np.ones((2, 12))))
    assert _solve(cx, _opts(), False) == before
    cx.close()


def test_refused_on_a_column_split_context(built):
    import lp_amd
    from lp_amd import _capi
    cx = lp_amd.Context(0)
    coll = _Collective()
    cx.set_collective(1, 2, coll)                                      # one rank of a column split over two
    m, n = 40, 100
    d, keep = _descriptor(T(_mat(97, m, n)), T(np.ones(m)), T(np.ones(n)))
    assert _capi.lib().lpipm_upload_device(cx._h, C.byref(d)) == _capi.ERR_UNSUPPORTED
    assert cx.resident_bytes() == 0
    b0, c0, k0 = _member(41, *SL, 2)                                   # a plain host upload is still taken, and stays
    cx.upload_arrays(_slack_form(*_blocks(41, *SL)), b0, _slack_cost(c0, SL[0]), k0, 24)
    before, held = _solve(cx, _opts(), False), cx.resident_bytes()
    assert _capi.lib().lpipm_upload_device(cx._h, C.byref(d)) == _capi.ERR_UNSUPPORTED
    assert cx.resident_bytes() == held and _solve(cx, _opts(), False) == before and before[0][0] == 0
    cx.set_collective(0, 1, None)                                      # the same context without the split takes it
    assert _capi.lib().lpipm_upload_device(cx._h, C.byref(d)) == _capi.OK
    cx.close()


# ---- 6. lp_amd.batch.solve_device ------------------------------------------------------------------------------------------------------
def _assert_rows(out, want):
    x, status, fun, its = out
    x = x.cpu().numpy()
    for k, (rc, xb, fb, it) in enumerate(want):
        assert (int(status[k]), int(its[k])) == (rc, it), k
        if xb is None:
            assert np.isnan(x[k]).all() and np.isnan(fun[k]), k
        else:
            assert _bits(x[k]).tobytes() == xb and _bits(fun[k]).tobytes() == fb, k


def test_solve_device_members_that_own_their_matrices(built):
    import lp_amd
    from lp_amd import batch
    K = 7
    mats = [_slack_form(*_blocks(50 + k, *SL)) for k in range(K)]
    mem = [_member(50 + k, *SL, k, infeasible=(k == INF)) for k in range(K)]
    bs, cs, c0s = [m[0] for m in mem], [_slack_cost(m[1], SL[0]) for m in mem], [m[2] for m in mem]
    host = lp_amd.Context(0)
    want = []
    for k in range(K):
        host.upload_arrays(mats[k], bs[k], cs[k], c0s[k], 24)
        want.append(_norm(*host.solve_raw(_opts())[:4]))
    host.close()
    cx = lp_amd.Context(0)
    out = batch.solve_device(T(np.stack(mats)), T(np.stack(bs)), T(np.stack(cs)), c0s, n_slack=24, ctx=cx, max_group=3)
    _assert_rows(out, want)
    assert want[INF][0] == 5 and [w[0] for i, w in enumerate(want) if i != INF] == [0] * (K - 1)
    cx.close()


def test_solve_device_tall_members_over_one_matrix(built):
    import lp_amd
    from lp_amd import batch
    K = 7
    A_ub, _ = _blocks(46, *TL)
    mem = _members(TL, 46, K)
    bs, cs = [m[0] for m in mem], [m[1] for m in mem]
    host = lp_amd.Context(0)
    want = []
    for k in range(K):
        host.upload(lp_amd.Problem.target(cs[k]).ub(A_ub, bs[k]).build(), tall=True)
        want.append(_norm(*host.solve_raw(_opts())[:4]))
    host.close()
    cx = lp_amd.Context(0)
    out = batch.solve_device(T(A_ub.T.copy()).t(), T(np.stack(bs)), T(np.stack(cs)), form="ub_tall", ctx=cx, max_group=3)
    _assert_rows(out, want)
    assert want[INF][0] == 5
    cx.close()
