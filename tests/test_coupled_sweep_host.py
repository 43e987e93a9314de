"""The plan of the coupled sweep without a device (lpipm_k_sweep_plan): for nsb = 1 .. 5 super-blocks, a partial last one
included, the launches, their pieces, the workgroup cuts between pieces, and which coupling blocks exist.

  F_0: y_0 = Inv_0 r_0                     F_k (0 < k < nsb-1): y_k = Inv_k t_k - G_k y_k-1  ||  t_j -= L[j,k-1] y_k-1, j > k
  F_nsb-1: two launches                    B_nsb-1: v = Inv^T y        B_k: v_k = Inv_k^T s_k - H_k v_k+1  ||  one piece per i < k
"""
import ctypes as C

import pytest

# (m, super-block width) -> widths of the super-blocks
SHAPES = [(512, 512), (1000, 512), (1536, 512), (1400, 512), (2048, 512), (4096, 1024), (2500, 512), (4500, 1024)]


def _plan(m, w, coupled=1):
    from lp_amd import _capi
    out = (C.c_int32 * 4096)()
    n, nbytes = C.c_int32(0), C.c_uint64(0)
    rc = _capi.lib().lpipm_k_sweep_plan(m, w, coupled, out, 4096, C.byref(n), C.byref(nbytes))
    assert rc == 0
    return list(out[:n.value]), nbytes.value


def _widths(m, w):
    mp = -(-m // 128) * 128
    return mp, [min(w, mp - r) for r in range(0, mp, w)]


def _parse(v):
    nsb, coupled, nl = v[0], v[1], v[2]
    at, launches = 3, []
    for _ in range(nl):
        kind, k, npieces, blocks = v[at:at + 4]
        at += 4
        pieces = []
        for _ in range(npieces):
            pieces.append(dict(zip(("rows", "np0", "np1", "w0", "w0_y", "w1", "w1_y", "add", "add_y", "out", "out_y", "blk0"), v[at:at + 12])))
            at += 12
        launches.append((kind, k, blocks, pieces))
    couple = [tuple(v[at + 4 * i:at + 4 * i + 4]) for i in range(nsb)] if coupled else []
    assert at + 4 * len(couple) == len(v)
    return nsb, coupled, launches, couple


@pytest.mark.parametrize("m,w", SHAPES)
def test_plan_pieces_and_cuts(built, m, w):
    mp, s = _widths(m, w)
    row0 = [sum(s[:k]) for k in range(len(s))]
    v, nbytes = _plan(m, w)
    nsb, coupled, launches, couple = _parse(v)
    assert nsb == len(s)
    if nsb == 1:
        assert coupled == 0 and launches == [] and nbytes == 0      # falls back to the plain sweep
        return
    assert coupled == 1
    assert len(launches) == 2 * nsb + 1                               # nine at nsb = 4, where the plain sweep has seventeen
    fwd = [l for l in launches if l[0] == 0]
    bwd = [l for l in launches if l[0] == 1]
    assert [l[1] for l in fwd] == list(range(nsb - 1)) + [nsb - 1, nsb - 1]
    assert [l[1] for l in bwd] == list(range(nsb - 1, -1, -1))
    for kind, k, blocks, pieces in launches:
        cut = 0
        for p in pieces:                                              # a piece's workgroups: four rows each, in order
            assert p["blk0"] == cut
            cut += -(-p["rows"] // 4)
        assert blocks == cut
    R, Y = 0, 1
    for kind, k, blocks, pieces in fwd[:nsb - 1]:
        main = pieces[0]
        assert (main["rows"], main["np0"], main["w0"], main["w0_y"], main["add"], main["out"], main["out_y"]) == (s[k], s[k], row0[k], R, -1, row0[k], Y)
        if k == 0:
            assert len(pieces) == 1 and main["np1"] == 0
            continue
        assert (main["np1"], main["w1"], main["w1_y"]) == (s[k - 1], row0[k - 1], Y)            # - G_k y_k-1
        assert len(pieces) == 2
        far, below = pieces[1], row0[k] + s[k]
        assert (far["rows"], far["np0"], far["np1"], far["w0"], far["w0_y"]) == (mp - below, s[k - 1], 0, row0[k - 1], Y)
        assert (far["add"], far["add_y"], far["out"], far["out_y"]) == (below, R, below, R)
    k = nsb - 1
    (_, _, _, near), (_, _, _, last) = fwd[nsb - 1:]
    assert len(near) == 1 and len(last) == 1
    assert (near[0]["rows"], near[0]["np0"], near[0]["w0"], near[0]["w0_y"], near[0]["add"], near[0]["add_y"], near[0]["out"], near[0]["out_y"]) == \
        (s[k], s[k - 1], row0[k - 1], Y, row0[k], R, row0[k], R)
    assert (last[0]["rows"], last[0]["np0"], last[0]["np1"], last[0]["w0"], last[0]["w0_y"], last[0]["add"], last[0]["out"], last[0]["out_y"]) == \
        (s[k], s[k], 0, row0[k], R, -1, row0[k], Y)
    for kind, k, blocks, pieces in bwd:
        main = pieces[0]
        assert (main["rows"], main["np0"], main["w0"], main["w0_y"], main["add"], main["out"], main["out_y"]) == (s[k], s[k], row0[k], Y, -1, row0[k], R)
        if k == nsb - 1:
            assert len(pieces) == 1 and main["np1"] == 0
            continue
        assert (main["np1"], main["w1"], main["w1_y"]) == (s[k + 1], row0[k + 1], R)            # - H_k v_k+1
        assert len(pieces) == 1 + k
        for i, p in enumerate(pieces[1:]):                            # s_i -= L[k+1,i]^T v_k+1
            assert (p["rows"], p["np0"], p["np1"], p["w0"], p["w0_y"]) == (s[i], s[k + 1], 0, row0[k + 1], R)
            assert (p["add"], p["add_y"], p["out"], p["out_y"]) == (row0[i], Y, row0[i], Y)
    # coupling blocks: H_k for k < nsb-1, G_k for 1 <= k <= nsb-2 (never the last: it would wait for the last inverse), and the
    # transposed block column k from the near block where G_k+1 reads it, else from the first far block
    doubles = 0
    for k, (lt_row0, lt_ld, has_h, has_g) in enumerate(couple):
        assert has_h == (1 if k < nsb - 1 else 0)
        assert has_g == (1 if 1 <= k <= nsb - 2 else 0)
        j = k + 1 if k + 1 <= nsb - 2 else k + 2
        assert (lt_row0, lt_ld) == ((row0[j], mp - row0[j]) if j < nsb else (-1, 0))
        doubles += (s[k] * s[k + 1] if has_h else 0) + (s[k] * s[k - 1] if has_g else 0) + s[k] * lt_ld
    assert nbytes == 8 * doubles


def test_uncoupled_plan_lists_nothing(built):
    v, nbytes = _plan(4096, 1024, coupled=0)
    assert v == [4, 0, 0] and nbytes == 0


def test_headline_storage(built):
    """4096 rows, 1024-wide super-blocks, both sweeps: three H, two G, and block columns 0 (three blocks) and 1 (two)
    transposed.  The backward sweep alone (the default): three H and the far blocks, two of column 0 and one of column 1.
    The forward sweep alone: two G and the near blocks they read."""
    assert _plan(4096, 1024)[1] == 8 * 1024 * 1024 * (3 + 2 + 3 + 2)
    assert _plan(4096, 1024, coupled=2)[1] == 8 * 1024 * 1024 * (3 + 2 + 1)
    assert _plan(4096, 1024, coupled=3)[1] == 8 * 1024 * 1024 * (2 + 1 + 1)


@pytest.mark.parametrize("m,w", [(1536, 512), (4096, 1024), (4500, 1024)])
def test_parts_alone_list_their_own_sweep(built, m, w):
    mp, s = _widths(m, w)
    nsb = len(s)
    _, _, both, _ = _parse(_plan(m, w)[0])
    _, _, only_h, couple_h = _parse(_plan(m, w, coupled=2)[0])
    _, _, only_g, couple_g = _parse(_plan(m, w, coupled=3)[0])
    bwd, fwd = [l for l in only_h if l[0] == 1], [l for l in only_g if l[0] == 0]
    # the sweep that is not coupled: the plain recurrence, two launches per step (one for the last forward step); the plain
    # backward sweep stays with the transposed mat-vec and its fold and is not listed
    plain = [l for l in only_h if l[0] == 0]
    assert [l[1] for l in plain] == [k for k in range(nsb) for _ in range(2 if k < nsb - 1 else 1)]
    assert all(len(l[3]) == 1 and l[3][0]["np1"] == 0 for l in plain)
    assert [l for l in only_g if l[0] == 1] == []
    # the backward launches are the coupled ones (one per step); the pieces do not depend on which other sweep is coupled
    assert [l[:3] for l in bwd] == [l[:3] for l in both if l[0] == 1] and len(bwd) == nsb
    assert [l[:3] for l in fwd] == [l[:3] for l in both if l[0] == 0] and len(fwd) == nsb + 1
    assert all(g == 0 for _, _, _, g in couple_h) and all(h == 0 for _, _, h, _ in couple_g)
    for k, (lt_row0, lt_ld, _, _) in enumerate(couple_h):          # far blocks only
        assert (lt_row0, lt_ld) == ((sum(s[:k + 2]), mp - sum(s[:k + 2])) if k + 2 < nsb else (-1, 0))
    for k, (lt_row0, lt_ld, _, _) in enumerate(couple_g):          # the near block G_k+1 reads, nothing else
        assert (lt_row0, lt_ld) == ((sum(s[:k + 1]), s[k + 1]) if k + 1 <= nsb - 2 else (-1, 0))
