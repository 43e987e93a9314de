"""Lockstep batches on ONE shared constraint matrix (lpipm_upload_lockstep_shared) at every variant of the three passes
over a shared A (the SHARED instantiations of gemv_n_kernel, gemv_t_kernel, gemv_dual_kernel) and every layout of their
member groups.  Which branch a case reaches follows from the host-side rules, mirrored in _plan() and asserted by each test:

  mp = m rounded up to 128, npa = n rounded up to 16; a batch of 16 or more runs as two half-batch views of B / 2 and
  B - B / 2 members (the second with first != 0), and every rule below sees the VIEW's count;
  gemv_dual: 1024-column chunks and groups of 2 members from npa >= 4096 (8 column pairs per lane, 2 rows per trip),
             else 256-column chunks and groups of 4;
  gemv_n   : groups of 4; 4 rows per wave when m * groups > 2048 (a row tail when m is no multiple of 16), else 1;
  gemv_t   : groups of 8; mp / 128 row slabs;
  A.D.A^T  : chunks of 8 / 16 k-tiles up to 64 / 256 k-tiles (uniform), above that 1024-column chunks whose last is cut into
             quarters (non-uniform); a batch always takes the units kernel (member stride 0 for A), with 2 chunks per unit
             where the chunking is uniform, else 1; a single LP with more than 16 tiles, several chunks and fewer than 256
             (tile, chunk) units takes the stream-K kernel with its fix-up launch instead.

  m x n          count(s)       what it is there for
  333 x 4100     1 2 3 5        dual <1024, 2>: last chunk 16 columns wide; non-uniform A.D.A^T chunks (8), upc falls to 1
  512 x 4096     1 2 3 5        dual <1024, 2>, whole chunks; 16 uniform chunks, 2 per unit
  300 x 9000     1 2 3 5        dual <1024, 2>: 9 chunks, last one 808 columns; 3 row slabs
  1000 x 5000    1 2 3 5        dual <1024, 2>: 8 row slabs x 5 chunks; 36 tiles x 11 chunks
  700 x 1500     5 13           gemv_n RPW 1 and 4 on one A, 700 = 16 * 43 + 12; single LP: stream-K (21 tiles x 6 chunks)
  1009 x 1100    5 9            the same, 1009 = 16 * 63 + 1; single LP: stream-K (36 tiles x 5 chunks), 5 chunks 2 per unit
  516 x 1100     5 13           the same, 516 = 16 * 32 + 4
  527 x 1200     5 13           the same, 527 = 16 * 32 + 15
  1100 x 2300    5              mp = 1152 > 1024: 9 row slabs, 9 dual chunk slabs, the multi-workgroup vector stage
  2100 x 4200    5              mp = 2176: 1024-wide super-blocks, 17 row slabs, npa >= 4096, RPW 4 with a tail (16 * 131 + 4)
  256 x 1100     7 .. 33        group layouts: last group of 2 / 4 / 8 short by every amount, one view and two (10 and
                                27 = 13 + 14 added to the issue's counts: without them no view is short by 2, 3 or 6)
  256 x 1100     13, 29         members that stop between 3 and 34 iterations, whole groups finished, mixed outcomes
  4096 x 8192, 300 x 140000     kernel hooks only (count 1 and 5)

References, in order of strength: (1) every member bit for bit the single solve of (A, b_i, c_i, c0_i) on a fresh context;
(2) bit for bit the same batch uploaded with one copy of A per member; (3) the CPU oracle: same status and iteration
count, |x - x_oracle| <= 1e-6 -- on members for which the oracle is pinned: its run on a column-permuted copy of the member
takes the same iteration count and agrees with the first run to 1e-7 (a tenth of the bound).  The kernel-level tests at the
end tell which pass is wrong when a solve-level case fails: the three GEMV hooks on a shared-uploaded context bit-equal to
the hooks on a single upload, and within oracle.vector_checks.check_gemv's componentwise bound of an extended-precision
reference.

That the file bites: six changes to kernels_gemv.hip, each built and run once on an MI355X against the shared-matrix tests
that existed before (tests/test_gpu_shared_matrix.py, the only other file that uploads a shared matrix) and against this
file (a record of that run; the kernels and launchers are named as they are named now):

  change                                                              before          this file
  1 launch_gemv_dual, shared 1024 branch: groups of 4 in the grid      passes          5 fail (dual x 4, 2100 x 4200)
  2 gemv_dual_kernel<1024, 2, true>: RG forced to 4                    passes          12 fail (those 5, 7 dual hooks)
  3 the same kernel: column sub-slab NS - 1 left out of cacc (NS = 8)  passes          12 fail (the same 12)
  4 gemv_n_kernel, groups of 4: if (row0 + RPW > m) return             passes          2 fail (RPW test at m = 1009 and 527)
  5 gemv_t_kernel, groups of 8: the store loop stops at SG_T - 1       3 of 10 fail    7 fail (RPW x 4, layouts, staggered x 2)
  6 group_load: the member after a finished one not live               7 of 10 fail    3 fail (staggered x 2, 1000 x 5000)

Wall time of this file on an MI355X box (16 CPUs): 53 s, against 74 s for tests/test_gpu_vector_stage_at_scale.py in the
same run of the suite (WALL_TIME below).
"""
import functools

import numpy as np
import pytest

from oracle import vector_checks as vc

pytestmark = pytest.mark.gpu

# Measured on an MI355X box inside one run of the whole suite: this file 53 s (58 s run alone), against 74 s for
# tests/test_gpu_vector_stage_at_scale.py, unchanged since the parent commit (the yardstick: this file should take no more than
# about twice that).  Most of it is the CPU oracle, twice per compared member: 15 s at 1000 x 5000, 10 s at 512 x 4096.
WALL_TIME = "53 s; tests/test_gpu_vector_stage_at_scale.py in the same run: 74 s"

OK, UNBOUNDED, ITERATION_LIMIT = 0, 6, 7
X_BOUND = 1e-6                   # |x - x_oracle|, the bound of every parity test of the suite
PIN_BOUND = 1e-7                 # the oracle against itself on the column-permuted member: a tenth of X_BOUND


def _up(v, k):
    return -(-v // k) * k


def _views(count):
    """[(first, count)] of the views a resident batch is solved as (solve_lockstep: two half-batches from 16 members)"""
    return [(0, count)] if count < 16 else [(0, count // 2), (count // 2, count - count // 2)]


def _plan(m, n, count=1):
    """The host-side launch rules (upload_impl, plan_adat, launch_gemv_* with shared_a, units_chunking) for one VIEW of
    `count` members."""
    mp, npa = _up(m, 128), _up(n, 16)
    KT = npa // 16
    kc = 8 if KT <= 64 else (16 if KT <= 256 else 64)
    if KT <= kc:
        cpt, uniform = 1, True
    elif KT <= 256:
        cpt, uniform = -(-KT // kc), True
    else:
        nbig, ks = KT // kc - 1, kc // 4
        cpt, uniform = nbig + -(-(KT - nbig * kc) // ks), False
    nt = mp // 128
    ntiles = nt * (nt + 1) // 2
    groups_n = -(-count // 4)
    return dict(mp=mp, npa=npa, cw=1024 if npa >= 4096 else 256, sg_dual=2 if npa >= 4096 else 4,
                dual_chunks=-(-npa // 1024) if npa >= 4096 else -(-npa // 256), row_slabs=mp // 128,
                rpw=1 if m * groups_n <= 2048 else 4, cpt=cpt, uniform=uniform, ntiles=ntiles,
                upc=1 if count == 1 or not uniform else min(cpt, 2),
                single_streamk=cpt > 1 and ntiles > 16 and ntiles * cpt < 256)


def _norm(rc, x, fun, it):
    has_x = rc in (OK, ITERATION_LIMIT)
    return (int(rc), x if has_x else None, fun if has_x else None, int(it))


def _same_member(i, a, b, what):
    """two (status, x | None, fun, iterations) agree bit for bit"""
    assert a[0] == b[0] and a[3] == b[3], (what, i, "status", a[0], b[0], "iterations", a[3], b[3])
    assert (a[1] is None) == (b[1] is None), (what, i)
    if a[1] is not None:
        assert np.array_equal(a[1], b[1]), (what, i, float(np.abs(a[1] - b[1]).max()))
        assert a[2] == b[2], (what, i, a[2], b[2])


class _Family:
    """kmax members on one A.  Batches of every count take the first `count` of them, so a member's single solve and its
    oracle runs are done once."""

    def __init__(self, seed, m, n, kmax, spreads=None):
        from lp_amd import synth
        self.seed, self.m, self.n, self.kmax = seed, m, n, kmax
        if spreads is None:
            self.A, self.bs, self.cs, self.xstars = synth.planted_scenarios(seed, m, n, kmax)
        else:
            assert len(spreads) == kmax
            self.A, self.bs, self.cs, self.xstars = synth.spread_scenarios(seed, m, n, spreads)
        self.c0s = [0.25 * i for i in range(kmax)]
        self._single, self._oracle = {}, {}

    def single(self, i, o):
        """(status, x | None, fun, iterations) of member i solved alone on a fresh context"""
        import lp_amd
        key = (i, int(o.max_iter))
        if key not in self._single:
            c = lp_amd.Context(0)
            c.upload_arrays(self.A, self.bs[i], self.cs[i], self.c0s[i])
            rc, x, fun, it, _ = c.solve_raw(o)
            c.close()
            self._single[key] = _norm(rc, x, fun, it)
        return self._single[key]

    def oracle(self, i, max_iter=None):
        """the CPU oracle on member i (status and iteration count; with x for an optimal member)"""
        from oracle import capi as oracle
        key = (i, max_iter)
        if key not in self._oracle:
            opts = oracle.default_opts() if max_iter is None else oracle.default_opts(max_iter=max_iter)
            self._oracle[key] = oracle.solve(self.A, self.bs[i], self.cs[i], self.c0s[i], opts, want_log=False)
        return self._oracle[key]

    def pinned_oracle(self, i):
        """oracle(i), after showing that the oracle is pinned on this member: its run on the column-permuted member takes the
        same iteration count and agrees to PIN_BOUND.  A member that is not pinned asks for another seed, not another bound."""
        from oracle import capi as oracle
        key = ("pin", i)
        if key not in self._oracle:
            ref = self.oracle(i)
            P = np.random.default_rng([self.seed, i]).permutation(self.n)
            alt = oracle.solve(np.ascontiguousarray(self.A[:, P]), self.bs[i], self.cs[i][P], self.c0s[i], want_log=False)
            assert ref["status"] == alt["status"] == OK, (i, ref["status"], alt["status"])
            assert ref["iterations"] == alt["iterations"], ("oracle not pinned", i, ref["iterations"], alt["iterations"])
            d = float(np.abs(ref["x_slack"][P] - alt["x_slack"]).max())
            assert d <= PIN_BOUND, ("oracle not pinned", i, d)
            self._oracle[key] = d
        return self.oracle(i)


@functools.lru_cache(maxsize=1)
def _family(seed, m, n, kmax, spreads=None):
    return _Family(seed, m, n, kmax, spreads)


def _oracle_members(count):
    """the first, the last, and one that is not first in its group of 2, 4 or 8 (index 3 mod 8); all of a batch up to 3"""
    return sorted({0, count - 1} | ({3} if count > 3 else set(range(count))))


def _check_batch(ctx, fam, count, o, oracle_members=(), copies=True, what=""):
    """Members [0, count) of fam as one shared batch on ctx: (1) singles, all members; (2) copies; (3) the oracle.
    -> the batch's results"""
    import lp_amd
    A, bs, cs, c0s = fam.A, fam.bs[:count], fam.cs[:count], fam.c0s[:count]
    ctx.upload_lockstep_shared(A, bs, cs, c0s)
    res = [_norm(*r) for r in ctx.solve_lockstep(o)]
    print(f"\n[measure] {what} {fam.m}x{fam.n} count {count}: status {[r[0] for r in res]} iterations {[r[3] for r in res]}")
    for i in range(count):
        _same_member(i, res[i], fam.single(i, o), f"{what} count {count}: shared vs single")
    if copies:
        assert count * fam.m * fam.n * 8 <= 4 << 30                      # above 4 GB of copies this path is left out
        cp = lp_amd.Context(0)
        cp.upload_lockstep([A] * count, bs, cs, c0s)
        rc = [_norm(*r) for r in cp.solve_lockstep(o)]
        cp.close()
        for i in range(count):
            _same_member(i, res[i], rc[i], f"{what} count {count}: shared vs copies")
    for i in oracle_members:
        ref = fam.pinned_oracle(i)
        st, x, fun, it = res[i]
        assert st == ref["status"] == OK and it == ref["iterations"], (what, count, i, st, it, ref["status"], ref["iterations"])
        err = float(np.abs(x - ref["x_slack"]).max())
        print(f"[measure] {what} count {count} member {i}: {it} iterations, |x - x_oracle| = {err:.3g}")
        assert err <= X_BOUND, (what, count, i, err)
    return res


def _default_opts():
    import lp_amd
    return lp_amd.InteriorPoint.default().opts()


# ---------------------------------------------------------------------------------------------------------------------
# launch_gemv_dual with shared_a, npa >= 4096: gemv_dual_kernel<1024, 2, true>
DUAL_SHAPES = [(333, 4100, 11), (512, 4096, 12), (300, 9000, 13), (1000, 5000, 115)]


@pytest.mark.parametrize("m,n,seed", DUAL_SHAPES)
def test_dual_pass_1024_columns_groups_of_two(ctx, m, n, seed):
    """Counts 1, 2, 3 and 5: the group of 2 short, full, short after a full one, short after two full ones."""
    p = _plan(m, n)
    assert p["npa"] >= 4096 and p["cw"] == 1024 and p["sg_dual"] == 2
    if (m, n) != (512, 4096):
        assert p["npa"] % 1024 != 0 and p["npa"] % 128 != 0                     # the last chunk and its last sub-slab partial
    if (m, n) == (333, 4100):
        # A.D.A^T past 4096 columns: non-uniform chunks, one per unit although the batch would take two
        assert not p["uniform"] and p["cpt"] == 8 and _plan(m, n, 5)["upc"] == 1
    if (m, n) == (512, 4096):
        assert p["uniform"] and p["cpt"] == 16 and _plan(m, n, 5)["upc"] == 2
    if (m, n) == (1000, 5000):
        # 36 tiles x 11 chunks: 8 row slabs of the dual pass times 5 chunk slabs.  (With the chunking of units_chunking
        # a single LP of this shape has 396 units and takes the units kernel too; the shapes where the single LP takes the
        # stream-K kernel with its fix-up and the batch the units kernel are 700 x 1500 and 1009 x 1100 below.)
        assert p["ntiles"] == 36 and p["cpt"] == 11 and not p["single_streamk"] and p["row_slabs"] == 8
    fam = _family(seed, m, n, 5)
    o = _default_opts()
    for count in (1, 2, 3, 5):
        groups = -(-count // 2)
        assert (count % 2 == 1) == (count in (1, 3, 5)) and groups == {1: 1, 2: 1, 3: 2, 5: 3}[count]
        _check_batch(ctx, fam, count, o, _oracle_members(count), what="dual<1024,2>")


# ---------------------------------------------------------------------------------------------------------------------
# launch_gemv_n with shared_a: 4 rows per wave with a row tail, and 1 row per wave, on one A
RPW_SHAPES = [(700, 1500, 121, 13), (1009, 1100, 22, 9), (516, 1100, 23, 13), (527, 1200, 124, 13)]


@pytest.mark.parametrize("m,n,seed,big", RPW_SHAPES)
def test_gemv_n_rows_per_wave_both_sides_of_the_threshold(ctx, m, n, seed, big):
    small = 5
    assert m % 16 in (1, 4, 12, 15)
    assert big < 16 and small < 16                                                  # one view each: the count is the launch's
    assert m * -(-big // 4) > 2048 and m % 16 != 0 and _plan(m, n, big)["rpw"] == 4    # RPW = 4, the last workgroup's rows past m
    assert m * -(-small // 4) <= 2048 and _plan(m, n, small)["rpw"] == 1
    p = _plan(m, n, big)
    if (m, n) in ((700, 1500), (1009, 1100)):
        # A.D.A^T with member stride 0 in the units kernel where the single LP takes the stream-K kernel and its fix-up
        assert p["single_streamk"] and p["uniform"] and p["upc"] == 2
    if (m, n) == (1009, 1100):
        assert p["cpt"] == 5                                                          # 2 chunks per unit, odd chunk count
    fam = _family(seed, m, n, big)
    o = _default_opts()
    _check_batch(ctx, fam, big, o, _oracle_members(big), what="gemv_n RPW 4")
    _check_batch(ctx, fam, small, o, _oracle_members(small), what="gemv_n RPW 1")


# ---------------------------------------------------------------------------------------------------------------------
# mp > 1024 and mp > 2048 in a shared batch
def test_many_row_slabs_1100x2300(ctx):
    m, n, count = 1100, 2300, 5
    p = _plan(m, n, count)
    assert p["mp"] == 1152 > 1024 and p["row_slabs"] == 9 and p["dual_chunks"] == 9 and p["cw"] == 256 and p["rpw"] == 4
    assert -(-max(m, n) // 256) > 4                                                   # the multi-workgroup vector stage
    fam = _family(31, m, n, count)
    _check_batch(ctx, fam, count, _default_opts(), _oracle_members(count), what="mp 1152")


def test_super_blocks_2100x4200(ctx):
    """mp = 2176: the factorisation's 1024-wide super-blocks, 17 row slabs of gemv_t / gemv_dual, the 1024-column dual pass
    and gemv_n's 4 rows per wave with a tail, all in one batch.  Singles and copies only (the single path at this size is held
    to references by the factor and vector-stage files)."""
    m, n, count = 2100, 4200, 5
    p = _plan(m, n, count)
    assert p["mp"] == 2176 > 2048 and p["row_slabs"] == 17 and p["npa"] >= 4096 and p["cw"] == 1024
    assert p["rpw"] == 4 and m % 16 == 4 and not p["uniform"] and p["upc"] == 1
    fam = _family(32, m, n, count)
    res = _check_batch(ctx, fam, count, _default_opts(), (), what="mp 2176")
    assert all(r[0] == OK for r in res)


# ---------------------------------------------------------------------------------------------------------------------
# group_load: every short last group, one view and two
LAYOUT_COUNTS = (7, 9, 10, 15, 16, 17, 23, 27, 33)


def test_group_layouts(ctx):
    """One view below 16 members, two half-batch views from 16 (the second with first != 0); over the counts the last group
    of 2, 4 and 8 members is short by every possible amount.  Singles only, every member."""
    m, n = 256, 1100
    short = {2: set(), 4: set(), 8: set()}
    for count in LAYOUT_COUNTS:
        views = _views(count)
        assert (len(views) == 1) == (count < 16)
        if count >= 16:
            assert views[1][0] == count // 2 != 0 and views[0][1] + views[1][1] == count
        for first, cnt in views:
            for sg in short:
                if cnt % sg:
                    short[sg].add((sg - cnt % sg, first != 0))
    for sg in short:                                               # short by 1 .. sg - 1, and at least once in a second view
        assert {d for d, _ in short[sg]} == set(range(1, sg)), (sg, short[sg])
        assert any(second for _, second in short[sg]), sg
    fam = _family(41, m, n, max(LAYOUT_COUNTS))
    o = _default_opts()
    for count in LAYOUT_COUNTS:
        res = _check_batch(ctx, fam, count, o, (), copies=False, what="layout")
        assert all(r[0] == OK for r in res)


# ---------------------------------------------------------------------------------------------------------------------
# members that stop at different iterations, at real size
def _unbounded_direction(A):
    """d >= 0 with A d = 0 (n > 2 m Gaussian columns have one): the oracle's solution of the feasibility LP
    A d = 0, sum d = 1, d >= 0."""
    from oracle import capi as oracle
    m, n = A.shape
    r = oracle.solve(np.vstack([A, np.ones((1, n))]), np.concatenate([np.zeros(m), [1.0]]), np.zeros(n), want_log=False)
    assert r["status"] == OK
    return np.maximum(r["x_slack"], 0.0)


# spread s of member i (magnitudes of x* and z* over 10^(+-s)); "U": an unbounded member.  By view (see _staggered_checks).
STAGGERED = {
    13: [0, 0, 0, 0, 0, 0, 0, 0,   1.5, 0.5, 2, 3,   0],
    29: [2, 0.5, "U", 1.5, 0, 1, 3, 1, 0.5, 2.5, "U", 1.5, 1, 0,
         0, 0, 0, 0, 0, 0, 0, 0,   1.5, 0.5, 2, 3,   1, "U", 0],
}


def _staggered_family(count):
    lay = STAGGERED[count]
    fam = _family(53, 256, 1100, count, tuple(0.0 if s == "U" else float(s) for s in lay))
    if not getattr(fam, "unbounded_done", False):
        d = _unbounded_direction(fam.A)
        for i, s in enumerate(lay):
            if s == "U":                                      # c.d < 0 along a feasible ray: unbounded
                c = fam.cs[i]
                fam.cs[i] = c - 2.0 * (c @ d) / (d @ d) * d
                assert fam.cs[i] @ d < 0
        fam.unbounded_done = True
    return fam, lay


@pytest.mark.parametrize("count", sorted(STAGGERED))
def test_members_stop_at_different_iterations(ctx, count):
    """(a) at least three iteration counts; (b) eight consecutive members, aligned to 8 within their view, all at least two
    iterations before the batch's last member: a whole group of every kernel returns early; (c) a finished member between
    two running ones inside a group of 4; (d) the last member of a short last group -- the one the group's empty places
    stand on -- finishes first.  All four from the CPU oracle's counts, before the device's results are looked at.  Then the
    same batch with max_iter between the counts (OK / UNBOUNDED / ITERATION_LIMIT side by side) and through
    solve_lockstep_device."""
    import torch
    import lp_amd
    fam, lay = _staggered_family(count)
    m, n = fam.m, fam.n
    assert m >= 256 and n >= 1100
    refs = [fam.oracle(i) for i in range(count)]
    its = [r["iterations"] for r in refs]
    want_status = [UNBOUNDED if s == "U" else OK for s in lay]
    assert [r["status"] for r in refs] == want_status
    print(f"\n[measure] staggered count {count}: oracle iterations {its}")
    first, cnt = _views(count)[-1]                                # the last view: first != 0 when there are two
    assert (first != 0) == (count >= 16)
    v = its[first:first + cnt]
    assert len(set(its)) >= 3                                                                        # (a)
    assert cnt > 8 and max(v[0:8]) <= max(its) - 2 and max(v[0:8]) <= max(v) - 2                         # (b)
    assert v[9] < v[8] and v[9] < v[10] and 8 % 4 == 0                                                   # (c)
    assert all(cnt % sg != 0 for sg in (2, 4, 8))                                                        # (d) short for 2, 4, 8
    assert all(v[-1] < v[j] for j in range(cnt - cnt % 8, cnt - 1))                   # first of its group of 8 (so of 4 and 2)

    o = _default_opts()
    # (3) on three optimal members of spread <= 1.5 (beyond that the oracle's own distance to x* passes 1e-6)
    # (chosen by spread, not by position: the first member of each spread 0.5, 1 and 1.5 that the batch has, and the last)
    chosen = {lay.index(s) for s in (0.5, 1, 1.5) if s in lay} | {count - 1}
    assert len(chosen) >= 3 and all(lay[i] != "U" and lay[i] <= 1.5 for i in chosen)
    res = _check_batch(ctx, fam, count, o, sorted(chosen), what="staggered")
    assert [r[0] for r in res] == want_status and [r[3] for r in res] == its

    # mixed outcomes: max_iter between the counts
    limit = 12
    assert min(its) < limit < max(its)
    ol = lp_amd.InteriorPoint.custom().max_iter(limit).build().opts()
    resl = _check_batch(ctx, fam, count, ol, (), what=f"staggered max_iter {limit}")
    for i, (st, x, fun, it) in enumerate(resl):
        ref = fam.oracle(i, limit)
        assert st == ref["status"] and it == ref["iterations"], (i, st, it, ref["status"], ref["iterations"])
    assert {r[0] for r in resl} == ({OK, UNBOUNDED, ITERATION_LIMIT} if "U" in lay else {OK, ITERATION_LIMIT})

    # the resident batch through solve_lockstep_device: rows of members without a solution untouched
    stride = n + 5
    out = torch.full((count, stride), -123.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev = ctx.solve_lockstep_device(ol, out.data_ptr(), stride)
    torch.cuda.synchronize()
    rows = out.cpu().numpy()
    for i, (st, fun, it) in enumerate(dev):
        assert st == resl[i][0] and it == resl[i][3], i
        if st in (OK, ITERATION_LIMIT):
            assert np.array_equal(rows[i, :n], resl[i][1]) and fun == resl[i][2], i
            assert np.all(rows[i, n:] == -123.0), i
        else:
            assert np.all(rows[i] == -123.0), i


# ---------------------------------------------------------------------------------------------------------------------
# the three passes by themselves: hooks on a shared-uploaded context (they work on member 0, a group holding one member)
HOOK_SHAPES = [(m, n) for m, n, _ in DUAL_SHAPES] + [(m, n) for m, n, _, _ in RPW_SHAPES] + \
              [(1100, 2300), (2100, 4200), (256, 1100), (4096, 8192), (300, 140000)]


@pytest.mark.parametrize("m,n", HOOK_SHAPES)
def test_gemv_hooks_on_shared_upload(built, m, n):
    """lpipm_k_gemv_n / _t / _dual on a context uploaded with upload_lockstep_shared (count 1 and count 5) run
    the SHARED instantiations of gemv_n_kernel / gemv_t_kernel / gemv_dual_kernel: bit-equal to the hooks on a single upload of the
    same A, and inside the componentwise bound 2 k u |A| |w| of the extended-precision reference."""
    import lp_amd
    from lp_amd import synth
    A = synth.planted_lp(60, m, n)[0]
    rng = np.random.default_rng([60, m, n])
    W = rng.standard_normal((2, n)) * np.exp(rng.uniform(-3, 3, (2, n)))
    V = rng.standard_normal((2, m)) * np.exp(rng.uniform(-3, 3, (2, m)))
    bs = [rng.standard_normal(m) for _ in range(5)]
    cs = [rng.standard_normal(n) for _ in range(5)]
    p = _plan(m, n)
    assert p["rpw"] == (4 if m > 2048 else 1)                         # the hooks launch one group

    def hooks(c):
        out = {}
        for nrhs in (2, 1):
            out["n", nrhs] = c.k_gemv_n(W[:nrhs])[0]
            out["t", nrhs] = c.k_gemv_t(V[:nrhs])[0]
        out["dual"] = c.k_gemv_dual(W[0], V[0])[:2]
        return out

    single = lp_amd.Context(0)
    single.upload_arrays(A, bs[0], cs[0])
    want = hooks(single)
    single.close()
    (yn, mn), (yt, mt) = vc.gemv_n_ref(A, W), vc.gemv_t_ref(A, V)
    worst = 0.0
    for count in (1, 5):
        sh = lp_amd.Context(0)
        sh.upload_lockstep_shared(A, bs[:count], cs[:count])
        got = hooks(sh)
        sh.close()
        for nrhs in (2, 1):
            assert np.array_equal(got["n", nrhs], want["n", nrhs]), (count, "gemv_n", nrhs)
            assert np.array_equal(got["t", nrhs], want["t", nrhs]), (count, "gemv_t", nrhs)
            worst = max(worst, vc.check_gemv(got["n", nrhs], yn[:nrhs], mn[:nrhs], n, f"shared gemv_n nrhs={nrhs} count={count}"))
            worst = max(worst, vc.check_gemv(got["t", nrhs], yt[:nrhs], mt[:nrhs], m, f"shared gemv_t nrhs={nrhs} count={count}"))
        assert np.array_equal(got["dual"][0], want["dual"][0]), (count, "gemv_dual A.w")
        assert np.array_equal(got["dual"][1], want["dual"][1]), (count, "gemv_dual A^T.v")
        worst = max(worst, vc.check_gemv(got["dual"][0], yn[:1], mn[:1], n, f"shared dual A.w count={count}"))
        worst = max(worst, vc.check_gemv(got["dual"][1], yt[:1], mt[:1], m, f"shared dual A^T.v count={count}"))
    print(f"\n[measure] shared hooks {m}x{n}: CW {p['cw']}, {p['row_slabs']} row slabs, {p['dual_chunks']} chunk slabs, "
          f"worst ratio to the bound {worst:.3g}")
