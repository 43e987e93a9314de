"""lp_amd -- MI355X-native interior-point LP hot path behind the reference's own API.

Host-side mirror (Python, over the C ABI of include/lpipm.h) of the public interface of
sebasv/lp (crate `ripped` 0.1.1) for the one path this package accelerates:

    reference (Rust)                                   here
    -----------------------------------------------    ------------------------------------------
    Problem::target(&c).ub(&A,&b).eq(&A,&b).build()    Problem.target(c).ub(A, b).eq(A, b).build()
    InteriorPoint::default()                           InteriorPoint.default()
    InteriorPoint::custom().tol(..)...build()          InteriorPoint.custom().tol(..)...build()
    solver.solve(&problem) -> Result<OptimizeResult>   solver.solve(problem) -> OptimizeResult | raises
    res.x() / res.fun() / res.iteration()              res.x() / res.fun() / res.iteration()
    LinearProgramError::{Unconstrained, ...}           LinearProgramError subclasses of the same names

(src/linear_program.rs:24-170, src/solvers/mod.rs:12-49, src/solvers/interior_point/mod.rs:41-197,
src/error.rs:7-29.)  A Rust `Result::Err(e)` becomes a raised exception of the matching class.
All numerics run in liblpipm.so on the GPU; importing this package never imports oracle/.
"""
from __future__ import annotations

import ctypes as C
import enum

import numpy as np

from . import _capi

__all__ = ["Problem", "ProblemBuilder", "InteriorPoint", "InteriorPointBuilder", "EquationSolverType",
           "OptimizeResult", "Solver", "Context", "LinearProgramError", "Unconstrained",
           "NumericalProblem", "InvalidParameter", "IncompatibleInputDimensions", "Infeasible",
           "Unbounded", "IterationLimitExceeded", "BackendError"]


# ------------------------------------------------------------------------------ error.rs:7-29
class LinearProgramError(Exception):
    """error.rs:10-28.  `code` is the lpipm_status the C ABI returned."""
    code = -1

    def __init__(self, msg: str | None = None):
        super().__init__(msg if msg is not None else _capi.strerror(self.code))


class Unconstrained(LinearProgramError):
    code = _capi.UNCONSTRAINED


class NumericalProblem(LinearProgramError):
    code = _capi.NUMERICAL_PROBLEM


class InvalidParameter(LinearProgramError):
    code = _capi.INVALID_PARAMETER

    def __init__(self, what: str = ""):
        super().__init__(f"A parameter was set to an invalid value: {what}")


class IncompatibleInputDimensions(LinearProgramError):
    code = _capi.INCOMPATIBLE_DIMENSIONS


class Infeasible(LinearProgramError):
    code = _capi.INFEASIBLE


class Unbounded(LinearProgramError):
    code = _capi.UNBOUNDED


class IterationLimitExceeded(LinearProgramError):
    """error.rs:26-28: carries the best x / tau after the final iteration (mod.rs:237-239)."""
    code = _capi.ITERATION_LIMIT

    def __init__(self, x: np.ndarray):
        super().__init__()
        self.x = x


class BackendError(RuntimeError):
    """HIP/driver failure (status >= 100): no analogue in the reference; never silently ignored."""


_BY_CODE = {c.code: c for c in (Unconstrained, NumericalProblem, IncompatibleInputDimensions, Infeasible, Unbounded)}


def _raise_for(code: int, x=None):
    if code == _capi.OK:
        return
    if code == _capi.ITERATION_LIMIT:
        raise IterationLimitExceeded(x)
    if code == _capi.INVALID_PARAMETER:
        raise InvalidParameter("rejected by the backend")
    if code in _BY_CODE:
        raise _BY_CODE[code]()
    raise BackendError(f"lpipm status {code}: {_capi.strerror(code)} {_capi.last_error_detail()}")


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ptrs(arrays):
    """The C array of pointers to the (contiguous float64) arrays."""
    return (C.POINTER(C.c_double) * len(arrays))(*[_p(a) for a in arrays])


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _rows(a, length):
    """`a` as the 1 or 2 contiguous float64 rows of `length` entries a kernel entry reads (a vector is one row); any other shape
    is IncompatibleInputDimensions."""
    a = np.atleast_2d(_f64(a))
    if a.ndim != 2 or a.shape[0] not in (1, 2) or a.shape[1] != length:
        raise IncompatibleInputDimensions()
    return a


def _vec(a, length):
    a = _f64(a)
    if a.shape != (length,):
        raise IncompatibleInputDimensions()
    return a


def _square(M):
    M = _f64(M)
    if M.ndim != 2 or M.shape[0] != M.shape[1]:
        raise IncompatibleInputDimensions()
    return M


# ------------------------------------------------------------------------------ linear_program.rs
class Problem:
    """A linear program in slack form (linear_program.rs:24-30): min c'x st A x == b, x >= 0."""

    def __init__(self, A, b, c, c0, n_slack, parts=None, dtype=np.float64, upper=None, lower=None):
        self._A, self._b, self._c, self._c0, self._n_slack = A, b, c, float(c0), int(n_slack)
        # ProblemBuilder.upper: one entry per structural column, +inf where there is no bound (None: no bounds at all).
        # A(), b() and c() stay the slack form WITHOUT the bounds; Context.upload hands them to lpipm_upload_bounded.
        # ProblemBuilder.lower: likewise, -inf where there is no lower end (None: all 0).  With any lower that is not 0
        # Context.upload hands both to lpipm_upload_bounds; the results come back in these variables.
        self._upper = upper
        self._lower = lower
        none = np.zeros(0, dtype=np.int64)
        has_l = np.isfinite(lower) if lower is not None else True
        self._bounded = np.flatnonzero(np.isfinite(upper) & has_l) if upper is not None else none
        self._free = np.flatnonzero(np.isinf(upper) & np.isinf(lower)) if lower is not None else none
        # F of Problem<F> (linear_program.rs:24): float32 when every array the builder was given is float32 (the reference
        # infers F from its ndarray arguments), float64 otherwise.  A Problem<f32> is solved by InteriorPoint<f32>
        # (lpipm_solve_f32: every operation in f32, src/float.rs:42-43).
        self.dtype = np.dtype(dtype)
        # the `ub` / `eq` blocks the builder was given: (A_ub, b_ub, A_eq, b_eq, c).  With them the slack-form matrix
        # is assembled on the device (lpipm_upload_ub_eq) and the host copy below exists only if A() is asked for.
        self._parts = parts

    @staticmethod
    def target(c) -> "ProblemBuilder":          # linear_program.rs:37-39
        return ProblemBuilder(c)

    def A(self) -> np.ndarray:                   # :42-44
        if self._A is None:                      # lazily: [[A_ub, I], [A_eq, 0]] (:145-156)
            A_ub, _, A_eq, _, c = self._parts
            m_ub, m_eq, n = A_ub.shape[0], A_eq.shape[0], c.shape[0]
            A = np.zeros((m_ub + m_eq, n + m_ub), dtype=self.dtype)
            A[:m_ub, :n] = A_ub
            A[m_ub:, :n] = A_eq
            A[np.arange(m_ub), n + np.arange(m_ub)] = 1.0
            self._A = A
        return self._A

    def b(self) -> np.ndarray:                   # :47-49
        return self._b

    def c(self) -> np.ndarray:                   # :52-54
        return self._c

    def c0(self) -> float:                       # :57-59
        return self._c0

    def n_slack(self) -> int:
        return self._n_slack

    def upper(self):
        """The upper bounds of the structural columns (+inf: none), or None for a Problem without bounds."""
        return self._upper

    def lower(self):
        """The lower bounds of the structural columns (-inf: none), or None for a Problem built without .lower (all 0)."""
        return self._lower

    def n_bounded(self) -> int:
        """Columns with a finite lower and a finite upper end: the bound rows of the upload."""
        return int(self._bounded.shape[0])

    def n_free(self) -> int:
        """Columns with neither end: each adds one negative part x^- at the end of the upload's x_slack."""
        return int(self._free.shape[0])

    def _tail(self) -> int:
        # what follows the structural columns in the upload's column vectors: `ub` slacks, bound slacks w, negative parts x^-
        return self._n_slack + self.n_bounded() + self.n_free()

    def denormalize_x_into(self, x_slack: np.ndarray) -> np.ndarray:   # :65-69
        # (a bounded upload's x_slack ends with the bound slacks w, behind the `ub` slacks; general bounds: then x^-)
        return np.array(x_slack[: x_slack.shape[0] - self._tail()])

    def denormalize_duals(self, y: np.ndarray, z: np.ndarray):
        """The counterpart of denormalize_x_into for the duals of the slack form (Context.duals): the rows split as
        ProblemBuilder::build stacks them (linear_program.rs:145-158: the `ub` rows first, one slack column each, then the
        `eq` rows), z cut to the structural columns.  -> (y_ub, y_eq, reduced_costs)"""
        y, z = np.asarray(y), np.asarray(z)
        ns, nb = self._n_slack, self.n_bounded()      # (a bounded upload: the bound rows and their slack columns come last)
        return np.array(y[:ns]), np.array(y[ns: y.shape[0] - nb]), np.array(z[: z.shape[0] - self._tail()])

    def denormalize_bound_duals(self, z: np.ndarray) -> np.ndarray:
        """The multipliers v_j >= 0 of the bounds x_j <= u_j per structural column (0 where there is no bound), from the z
        of a bounded upload (Context.duals): the reduced costs of the bound slacks, which are its last entries.  The bound
        row's own multiplier is y_b = -v up to the dual residual, and d fun / d u_j = -v_j."""
        z = np.asarray(z)
        nb, nf = self.n_bounded(), self.n_free()      # (general bounds: the negative parts' z^- come behind v)
        v = np.zeros(z.shape[0] - self._tail())
        if nb:
            v[self._bounded] = z[z.shape[0] - nf - nb: z.shape[0] - nf]
        return v

    def denormalize_certificate(self, y, col, kind: int):
        """The counterpart of denormalize_duals for a certificate of the slack form (Context.certificate): the rows split as
        ProblemBuilder::build stacks them (the `ub` rows first, then the `eq` rows), col cut to the structural columns.
        Farkas (kind 1): -> (y_ub, y_eq, z) with A_ub^T y_ub + A_eq^T y_eq + z ~ 0, y_ub <= 0, z >= 0,
        b_ub.y_ub + b_eq.y_eq = 1.  Ray (kind 2; y is None): -> (None, None, x) with A_ub x <= 0, A_eq x ~ 0, x >= 0,
        c.x = -1.  No certificate (kind 0): -> (None, None, None)."""
        ns, nb = self._n_slack, self.n_bounded()      # (a bounded upload: the bound rows and their slack columns come last)
        if kind == _capi.CERT_NONE:
            return None, None, None
        col = np.asarray(col)
        cut = np.array(col[: col.shape[0] - self._tail()])
        if kind == _capi.CERT_RAY:
            return None, None, cut
        y = np.asarray(y)
        return np.array(y[:ns]), np.array(y[ns: y.shape[0] - nb]), cut

    def denormalize_bound_certificate(self, y, kind: int):
        """The bound rows' part of a Farkas ray of a bounded upload, per structural column (0 where there is no bound):
        y_upper <= 0 with A_ub^T y_ub + A_eq^T y_eq + y_upper + z ~ 0 and b_ub.y_ub + b_eq.y_eq + u.y_upper = 1 over the
        bounded columns.  None for any other kind, and for a Problem without bounds."""
        nb = self.n_bounded()
        if kind != _capi.CERT_FARKAS or nb == 0:
            return None
        y = np.asarray(y)
        out = np.zeros(self._upper.shape[0])
        out[self._bounded] = y[y.shape[0] - nb:]
        return out


class ProblemBuilder:
    """linear_program.rs:72-170."""

    def __init__(self, c):
        self._c = c
        self._ub = None
        self._eq = None
        self._upper = None
        self._lower = None

    def upper(self, u) -> "ProblemBuilder":
        """Upper bounds x_j <= u_j on the structural columns: one entry per column, +inf (np.inf) where there is none.
        The solves then run the bounded form (lpipm_upload_bounded): the normal matrix keeps its order.  Beside .lower a
        column may have an upper end only (lower -inf)."""
        self._upper = u
        return self

    def lower(self, l) -> "ProblemBuilder":
        """Lower bounds l_j <= x_j on the structural columns: one entry per column, -inf (-np.inf) where there is none;
        without this call every lower bound is 0.  A column with neither end is free.  The solves run lpipm_upload_bounds:
        shifts, reflections and free columns are handled in the vector stage, the normal matrix keeps its order and no
        column is stored twice; x, fun, the duals and the certificates come back in these variables."""
        self._lower = l
        return self

    def ub(self, A, b) -> "ProblemBuilder":      # :93-96
        self._ub = (A, b)
        return self

    def eq(self, A, b) -> "ProblemBuilder":      # :102-105
        self._eq = (A, b)
        return self

    def build(self) -> Problem:                  # :125-169
        given = [self._c] + [a for pair in (self._ub, self._eq) if pair is not None for a in pair]
        f32 = all(isinstance(a, np.ndarray) and a.dtype == np.float32 for a in given)
        c = _f64(self._c)
        if c.ndim != 1:
            raise IncompatibleInputDimensions()
        n = c.shape[0]
        A_ub, b_ub = self._ub if self._ub is not None else (np.zeros((0, n)), np.zeros(0))
        A_eq, b_eq = self._eq if self._eq is not None else (np.zeros((0, n)), np.zeros(0))
        A_ub, b_ub, A_eq, b_eq = _f64(A_ub), _f64(b_ub), _f64(A_eq), _f64(b_eq)
        if A_ub.ndim != 2 or A_eq.ndim != 2 or b_ub.ndim != 1 or b_eq.ndim != 1:
            raise IncompatibleInputDimensions()
        m_ub, m_eq = A_ub.shape[0], A_eq.shape[0]
        if m_ub + m_eq == 0:                                                 # :134-136
            raise Unconstrained()
        if (A_ub.shape[1] != A_eq.shape[1] or A_eq.shape[1] != n or m_ub != b_ub.shape[0]
                or m_eq != b_eq.shape[0]):                                   # :137-143
            raise IncompatibleInputDimensions()
        b = np.concatenate([b_ub, b_eq])                                     # :157-158
        cs = np.concatenate([c, np.zeros(m_ub)])                             # :159-160
        if self._upper is not None or self._lower is not None:   # (f64 whatever the arrays' type: the bounded forms have no f32 arm)
            upper = _f64(self._upper) if self._upper is not None else np.full(n, np.inf)
            if upper.shape != (n,):
                raise IncompatibleInputDimensions()
            if np.isnan(upper).any() or (upper == -np.inf).any():
                raise InvalidParameter("upper: NaN or -inf")
            lower = None
            if self._lower is not None:
                lower = _f64(self._lower)
                if lower.shape != (n,):
                    raise IncompatibleInputDimensions()
                if np.isnan(lower).any() or (lower == np.inf).any():
                    raise InvalidParameter("lower: NaN or +inf")
                lower = np.array(lower)
            return Problem(None, b, cs, 0.0, m_ub, parts=(A_ub, b_ub, A_eq, b_eq, c), upper=np.array(upper), lower=lower)
        if f32:     # Problem<f32>: the f32 values as given (exactly representable in the f64 working copies above)
            t = np.float32
            return Problem(None, b.astype(t), cs.astype(t), 0.0, m_ub,
                           parts=(A_ub.astype(t), b_ub.astype(t), A_eq.astype(t), b_eq.astype(t), c.astype(t)), dtype=t)
        return Problem(None, b, cs, 0.0, m_ub, parts=(A_ub, b_ub, A_eq, b_eq, c))   # :161; A on demand


# ------------------------------------------------------------------------------ solvers/mod.rs
class OptimizeResult:
    """solvers/mod.rs:19-49."""

    def __init__(self, x, fun, iteration):
        self._x, self._fun, self._iteration = x, float(fun), int(iteration)

    def iteration(self) -> int:
        return self._iteration

    def fun(self) -> float:
        return self._fun

    def x(self) -> np.ndarray:
        return self._x


class Solver:
    """solvers/mod.rs:12-16."""

    def solve(self, problem: Problem) -> OptimizeResult:
        raise NotImplementedError


class EquationSolverType(enum.IntEnum):
    """newton_equations.rs:37-46."""
    Cholesky = 0
    Inverse = 1
    LeastSquares = 2


def _batch_hints(problems):
    """The n_slack hints of [(A, b, c, c0[, n_slack]), ...] as a C array, or None when no member carries one."""
    ns = [int(p[4]) if len(p) > 4 and p[4] else 0 for p in problems]
    return (C.c_uint64 * len(ns))(*ns) if any(ns) else None


# ------------------------------------------------------------------------------ device context
def _tall_members(problems):
    """(A_ubs, b_ubs, cs, c0s) of Problems built from `ub` rows only -- the members of solve_batch(..., tall=True); anything
    else is a ValueError, raised before a context is touched."""
    members = []
    for p in problems:
        parts = getattr(p, "_parts", None)
        if parts is None or parts[2].shape[0] != 0:
            raise ValueError("tall=True needs Problems built from `ub` rows only")
        A_ub, b_ub, _, _, c = parts
        A_ub, b_ub, c = _f64(A_ub), _f64(b_ub), _f64(c)
        if A_ub.ndim != 2 or b_ub.shape != (A_ub.shape[0],) or c.shape != (A_ub.shape[1],):
            raise IncompatibleInputDimensions()
        members.append((A_ub, b_ub, c, float(p.c0())))
    return tuple(list(col) for col in zip(*members)) if members else ([], [], [], [])


def has_x(code) -> bool:
    """Whether a solve that ended with this status has a solution: x, and with it fun (mod.rs:231, :237-239)."""
    return code in (_capi.OK, _capi.ITERATION_LIMIT)


def _members_out(K, xs=None):
    """-> ((fun, iterations, status) C arrays of K members, unpack).  unpack(rc) raises for a failed call and else gives per
    member (status, x_slack | None, fun | None, iterations) -- x from the host rows xs -- or, without host rows,
    (status, fun | None, iterations)."""
    fun, its, st = (C.c_double * K)(), (C.c_uint64 * K)(), (C.c_int32 * K)()

    def unpack(rc):
        if rc != _capi.OK:
            _raise_for(rc)
        rows = zip(st, fun, its, [has_x(s) for s in st])              # (one pass over each C array: this sits in timed loops)
        if xs is None:
            return [(s, f if ok else None, t) for s, f, t, ok in rows]
        return [(s, x if ok else None, f if ok else None, t) for (s, f, t, ok), x in zip(rows, xs)]
    return (fun, its, st), unpack


def _solve_batch(ctx, problems, opts, tall, x_dev_ptr=None, row_stride=0):
    """One call of lpipm_solve_batch / _device / _slack / _ub_tall: host rows (x_dev_ptr None) or the device block.  The members
    are validated before the context is touched."""
    if tall:
        As, bs, cs, c0s = _tall_members(problems)
        ns = None
    else:
        As = [_f64(p[0]) for p in problems]; bs = [_f64(p[1]) for p in problems]; cs = [_f64(p[2]) for p in problems]
        for A, b, c in zip(As, bs, cs):
            if A.ndim != 2 or b.shape != (A.shape[0],) or c.shape != (A.shape[1],):
                raise IncompatibleInputDimensions()
        c0s = [float(p[3]) if len(p) > 3 else 0.0 for p in problems]
        ns = _batch_hints(problems)
    K = len(As)
    if K == 0:
        return []
    # a tall member's x has its m_ub slack values behind the n structural ones
    xs = [np.full(A.shape[1] + (A.shape[0] if tall else 0), np.nan) for A in As] if x_dev_ptr is None else None
    x_host, x_dev = (_ptrs(xs), None) if xs is not None else (None, C.c_void_p(int(x_dev_ptr)))
    m = (C.c_uint64 * K)(*[A.shape[0] for A in As]); n = (C.c_uint64 * K)(*[A.shape[1] for A in As])
    # (a member without rows has an empty matrix: any non-null pointer serves, its status is Unconstrained)
    members = (_ptrs(As), _ptrs(bs), _ptrs(cs), (C.c_double * K)(*c0s), C.byref(opts))
    out, unpack = _members_out(K, xs)
    L = _capi.lib()
    # the call replaces the context's resident problem with whatever it solved last: nothing the context recorded describes it
    ctx.m = ctx.n = ctx._m_eq = ctx._members = 0
    ctx._lock = None
    if tall:
        rc = L.lpipm_solve_batch_ub_tall(ctx._h, K, m, n, *members, x_host, x_dev, int(row_stride), *out)
    elif ns is not None:
        rc = L.lpipm_solve_batch_slack(ctx._h, K, m, n, ns, *members, x_host, x_dev, int(row_stride), *out)
    elif xs is not None:
        rc = L.lpipm_solve_batch(ctx._h, K, m, n, *members, x_host, *out)
    else:
        rc = L.lpipm_solve_batch_device(ctx._h, K, m, n, *members, x_dev, int(row_stride), *out)
    return unpack(rc)


_DEVICE_FORMS = {"slack": _capi.FORM_SLACK, "ub_eq": _capi.FORM_UB_EQ, "ub_tall": _capi.FORM_UB_TALL}


def _device_request(A, b, c, c0s=None, form="slack", A_eq=None, n_slack=0):
    """The lpipm_device_problem of torch CUDA tensors (Context.upload_device), checked without a context: shapes, one dtype
    (float64 or float32), one CUDA device.  -> (descriptor, what must stay alive while it is used, K, len(b[i]), len(x),
    device index, whether the request is a lockstep batch).  Tensors with a stride < 1 are made contiguous; nothing else is
    copied."""
    import torch
    if form not in _DEVICE_FORMS:
        raise ValueError(f"form must be one of {sorted(_DEVICE_FORMS)}")
    tensors = [A, b, c] + ([A_eq] if A_eq is not None else [])
    if not all(isinstance(t, torch.Tensor) for t in tensors):
        raise ValueError("upload_device takes torch tensors")
    if not all(t.is_cuda for t in tensors):
        raise ValueError("upload_device takes CUDA tensors: host arrays go through the upload* methods")
    if A.dtype not in (torch.float64, torch.float32) or any(t.dtype != A.dtype for t in tensors):
        raise ValueError("A, b, c (and A_eq) must all be float64 or all be float32")
    if any(t.device != A.device for t in tensors):
        raise ValueError("A, b, c (and A_eq) must be on one device")
    if (A_eq is not None and form != "ub_eq") or (n_slack and form != "slack") or int(n_slack) < 0:
        raise ValueError("A_eq belongs to form='ub_eq', n_slack to form='slack'")
    if A.ndim == 2 and b.ndim == 1:
        K, shared, batch = 1, 0, False
    elif A.ndim == 2 and b.ndim == 2:
        K, shared, batch = b.shape[0], 1, True
    elif A.ndim == 3 and b.ndim == 2:
        K, shared, batch = A.shape[0], 0, True
    else:
        raise IncompatibleInputDimensions()
    m, n = A.shape[-2:]
    m_eq = 0
    if A_eq is not None:
        if A_eq.ndim != 2 or A_eq.shape[1] != n:
            raise IncompatibleInputDimensions()
        m_eq = A_eq.shape[0]
    nb = m + m_eq
    if K < 1 or b.shape != ((K, nb) if batch else (nb,)) or c.shape != ((K, n) if batch else (n,)):
        raise IncompatibleInputDimensions()
    if c0s is not None and len(c0s) != K:
        raise IncompatibleInputDimensions()
    fix = lambda t: t if all(s >= 1 for s in t.stride()) else t.contiguous()
    A, b, c = fix(A), fix(b), fix(c)
    A_eq = fix(A_eq) if A_eq is not None else None
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
    mat = lambda t: _capi.DevMatrix(ptr(t), t.stride(-2), t.stride(-1), t.stride(0) if t.ndim == 3 else 0)
    vec = lambda t: _capi.DevVector(ptr(t), t.stride(-1), t.stride(0) if t.ndim == 2 else 0)
    c0 = (C.c_double * K)(*[float(v) for v in c0s]) if c0s is not None else None
    d = _capi.DeviceProblem(
        struct_size=C.sizeof(_capi.DeviceProblem), form=_DEVICE_FORMS[form], shared=shared, count=K, m=m, m_eq=m_eq, n=n,
        src_type=_capi.SRC_F32 if A.dtype == torch.float32 else _capi.SRC_F64, n_slack=int(n_slack), A=mat(A),
        A_eq=mat(A_eq) if A_eq is not None else _capi.DevMatrix(None, 1, 1, 0), b=vec(b), c=vec(c),
        c0=C.cast(c0, C.POINTER(C.c_double)) if c0 is not None else None)
    n_out = n if form == "slack" else n + m
    return d, (A, b, c, A_eq, c0), K, nb, n_out, A.device.index if A.device.index is not None else torch.cuda.current_device(), batch


class Context:
    """One lpipm_ctx: device buffers + stream of one (thread, device).  `InteriorPoint.solve` keeps one
    per device; bench/tests use it directly to separate the one-time upload from the timed solve."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        rc = _capi.lib().lpipm_create(int(device), C.byref(self._h))
        if rc != _capi.OK:
            raise BackendError(f"lpipm_create(device={device}) failed: {_capi.strerror(rc)}: "
                               f"{_capi.last_error_detail()} -- a HIP device is required, there is no CPU path")
        self.device = int(device)
        self.n = self.m = 0
        self._members = 1            # resident members: 1 after a single upload, the count of a lockstep batch
        self._m_eq = 0               # `eq` rows of the resident upload_tall_eq problem; every upload that succeeds sets it with m and n

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _capi.lib().lpipm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, problem: Problem, use_slack_structure: bool = True, tall: bool = False):
        """tall=True: the tall inequality form (lpipm_upload_ub_tall) -- a Problem with `ub` rows only, usually many more of
        them than columns; the solves then factor the n x n reduced system instead of the m x m normal matrix.  (A Problem
        that has `eq` rows as well: upload_tall_eq.)"""
        bounded = getattr(problem, "_upper", None) is not None and problem.n_bounded() > 0
        lower = getattr(problem, "_lower", None)
        general = lower is not None and bool(np.any(lower != 0.0))       # some lower end is not 0 (-inf included)
        if tall and (bounded or general):
            raise ValueError("tall=True does not take column bounds: on a tall form a bound is one more `ub` row")
        if general:
            # general bounds (lpipm_upload_bounds): x_slack = [x in the caller's variables; `ub` slacks; bound slacks; x^-]
            A_ub, b_ub, A_eq, b_eq, c = (_f64(a) for a in problem._parts)
            lower, upper = _f64(lower), _f64(problem._upper)
            m_ub, m_eq, n, nb, nf = A_ub.shape[0], A_eq.shape[0], c.shape[0], problem.n_bounded(), problem.n_free()
            rc = _capi.lib().lpipm_upload_bounds(self._h, n, m_ub, _p(A_ub) if m_ub else None, n, _p(b_ub) if m_ub else None,
                                                 m_eq, _p(A_eq) if m_eq else None, n, _p(b_eq) if m_eq else None,
                                                 _p(c), float(problem.c0()), _p(lower), _p(upper))
            _raise_for(rc)
            self.m, self.n, self._m_eq, self._members = m_ub + m_eq + nb, n + m_ub + nb + nf, 0, 1
            return self
        if bounded:
            # the bounded form (lpipm_upload_bounded): x_slack = [x; `ub` slacks; bound slacks], y = [y_ub; y_eq; y_bounds]
            A_ub, b_ub, A_eq, b_eq, c = (_f64(a) for a in problem._parts)
            upper = _f64(problem._upper)
            m_ub, m_eq, n, nb = A_ub.shape[0], A_eq.shape[0], c.shape[0], problem.n_bounded()
            rc = _capi.lib().lpipm_upload_bounded(self._h, n, m_ub, _p(A_ub) if m_ub else None, n, _p(b_ub) if m_ub else None,
                                                  m_eq, _p(A_eq) if m_eq else None, n, _p(b_eq) if m_eq else None,
                                                  _p(c), float(problem.c0()), _p(upper))
            _raise_for(rc)
            self.m, self.n, self._m_eq, self._members = m_ub + m_eq + nb, n + m_ub + nb, 0, 1
            return self
        if tall:
            parts = getattr(problem, "_parts", None)
            if parts is None or parts[0].shape[0] == 0 or parts[2].shape[0] != 0:
                raise ValueError("tall=True needs a Problem built from `ub` rows only")
            A_ub, b_ub, _, _, c = parts
            A_ub, b_ub, c = _f64(A_ub), _f64(b_ub), _f64(c)
            m_ub, n = A_ub.shape[0], c.shape[0]
            _raise_for(_capi.lib().lpipm_upload_ub_tall(self._h, n, m_ub, _p(A_ub), n, _p(b_ub), _p(c), float(problem.c0())))
            self.m, self.n, self._m_eq, self._members = m_ub, n + m_ub, 0, 1
            return self
        if use_slack_structure and getattr(problem, "_parts", None) is not None:
            # device-side assembly: the ub / eq blocks as given, no host slack matrix (lpipm_upload_ub_eq)
            A_ub, b_ub, A_eq, b_eq, c = problem._parts
            m_ub, m_eq, n = A_ub.shape[0], A_eq.shape[0], c.shape[0]
            rc = _capi.lib().lpipm_upload_ub_eq(self._h, n, m_ub, _p(A_ub) if m_ub else None, n, _p(b_ub) if m_ub else None,
                                                m_eq, _p(A_eq) if m_eq else None, n, _p(b_eq) if m_eq else None,
                                                _p(c), float(problem.c0()))
            _raise_for(rc)
            self.m, self.n, self._m_eq, self._members = m_ub + m_eq, n + m_ub, 0, 1
            return self
        A, b, c = _f64(problem.A()), _f64(problem.b()), _f64(problem.c())
        return self.upload_arrays(A, b, c, problem.c0(), problem.n_slack() if use_slack_structure else 0)

    def upload_tall_eq(self, problem: Problem):
        """The tall form with equality rows (lpipm_upload_ub_eq_tall): a Problem with `ub` rows -- usually many more of them
        than columns -- and any `eq` rows.  The solves factor the n x n reduced system of the `ub` rows and take the `eq` rows
        through a Schur complement on its factor; x_slack has n + m_ub entries, slack values last.  Without `eq` rows this is
        upload(problem, tall=True).  A Problem without `ub` rows is a ValueError (upload() is its entry)."""
        parts = getattr(problem, "_parts", None)
        if parts is None or parts[0].shape[0] == 0:
            raise ValueError("upload_tall_eq needs a Problem built from `ub` rows (and any `eq` rows)")
        A_ub, b_ub, A_eq, b_eq, c = (_f64(a) for a in parts)
        m_ub, m_eq, n = A_ub.shape[0], A_eq.shape[0], c.shape[0]
        rc = _capi.lib().lpipm_upload_ub_eq_tall(self._h, n, m_ub, _p(A_ub), n, _p(b_ub), m_eq, _p(A_eq) if m_eq else None, n,
                                                 _p(b_eq) if m_eq else None, _p(c), float(problem.c0()))
        _raise_for(rc)
        self.m, self.n, self._m_eq, self._members = m_ub + m_eq, n + m_ub, m_eq, 1
        return self

    def upload_arrays(self, A, b, c, c0=0.0, n_slack=0):
        A, b, c = _f64(A), _f64(b), _f64(c)
        if A.ndim != 2 or b.shape != (A.shape[0],) or c.shape != (A.shape[1],):
            raise IncompatibleInputDimensions()
        m, n = A.shape
        rc = _capi.lib().lpipm_upload_slack(self._h, m, n, _p(A), n, _p(b), _p(c), float(c0), int(n_slack))
        _raise_for(rc)
        self.m, self.n, self._m_eq, self._members = m, n, 0, 1
        return self

    def update_vectors(self, b, c):
        """New b and c for the resident single LP of upload_arrays (lpipm_update_vectors), in that upload's own form; A --
        and the first iteration's factor kept with it -- stays.  The next solve_raw is bit-identical to a fresh
        upload_arrays(A, b, c) + solve_raw."""
        b, c = _f64(b), _f64(c)
        if b.shape != (self.m,) or c.shape != (self.n,):
            raise IncompatibleInputDimensions()
        _raise_for(_capi.lib().lpipm_update_vectors(self._h, _p(b), _p(c)))
        return self

    def upload_device(self, A, b, c, c0s=None, *, form="slack", A_eq=None, n_slack=0):
        """A problem or a lockstep batch straight from torch CUDA tensors (lpipm_upload_device): float64 or float32 (all of one
        dtype), any strides, on this context's device; no host copy of A, b or c is made.  The shapes pick the request:
        A [m, n] with b [m]: a single LP; A [m, n] with b [K, .]: K members over ONE matrix; A [K, m, n]: K members that own
        their matrices.  form: "slack" (A with its slack columns, n_slack the hint of upload_arrays, verified on the device),
        "ub_eq" (A the `ub` rows, A_eq the `eq` rows, b = [b_ub; b_eq], c the structural costs) or "ub_tall" (`ub` rows
        only, the tall inequality form).  The context is then exactly where the equivalent host upload leaves it: solve_raw,
        solve_lockstep[_device], update_lockstep_vectors[_device] and scaling work unchanged, bit for bit.  Torch's current
        stream on the device is synchronised first; the tensors are free again when the call returns."""
        import torch
        d, keep, K, nb, n_out, dev, batch = _device_request(A, b, c, c0s, form, A_eq, n_slack)
        if dev != self.device:
            raise ValueError(f"the tensors are on device {dev}, the context on device {self.device}")
        torch.cuda.current_stream(dev).synchronize()         # the sources are complete when the library reads them
        _raise_for(_capi.lib().lpipm_upload_device(self._h, C.byref(d)))
        del keep
        if batch:
            self._lock = (K, nb, n_out, None, None, [np.empty(d.n)])     # (_lockstep_form reads the length of a c[i] from it)
        self.m, self.n, self._m_eq, self._members = nb, n_out, 0, K
        return self

    def update_vectors_device(self, b, c):
        """update_vectors with b [m] and c [n] taken from float64 torch CUDA tensors on this context's device
        (lpipm_update_vectors_device); non-contiguous ones are made contiguous on the device first."""
        import torch
        for t in (b, c):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64:
                raise ValueError("update_vectors_device takes float64 CUDA tensors")
        if b.shape != (self.m,) or c.shape != (self.n,):
            raise IncompatibleInputDimensions()
        if b.device.index != self.device or c.device.index != self.device:
            raise ValueError("the tensors are not on the context's device")
        b, c = b.contiguous(), c.contiguous()
        torch.cuda.current_stream(self.device).synchronize()
        _raise_for(_capi.lib().lpipm_update_vectors_device(self._h, C.c_void_p(b.data_ptr()), C.c_void_p(c.data_ptr())))
        return self

    def k_resident_matrix(self, member: int = 0):
        """-> the whole padded resident image (mp x npa) of the stored structural block of `member`, as the solves read it
        (lpipm_k_resident_matrix)."""
        mp, npa = C.c_uint64(0), C.c_uint64(0)
        _raise_for(_capi.lib().lpipm_k_resident_matrix(self._h, int(member), 0, 0, None, 0, C.byref(mp), C.byref(npa)))
        out = np.full((mp.value, npa.value), np.nan)
        _raise_for(_capi.lib().lpipm_k_resident_matrix(self._h, int(member), mp.value, npa.value, _p(out), npa.value, None, None))
        return out

    def k_pack_matrix(self, A, b, c, repeats=20, **kw):
        """-> (pack_ms, copy_ms): the launch that moved A of the resident upload_device(A, b, c, **kw), `repeats` times back to
        back between two events, and the runtime's device-to-device copy of as many bytes the same way (lpipm_k_pack_matrix)."""
        d, keep = _device_request(A, b, c, **kw)[:2]
        pack, copy = C.c_double(0.0), C.c_double(0.0)
        _raise_for(_capi.lib().lpipm_k_pack_matrix(self._h, C.byref(d), int(repeats), C.byref(pack), C.byref(copy)))
        del keep
        return pack.value, copy.value

    def _lockstep_form(self):
        """(members, len(b[i]), len(c[i])) of the resident lockstep batch, in its upload's own form."""
        lock = getattr(self, "_lock", None)
        if lock is None:
            raise BackendError("no lockstep batch is resident on this context")
        K, m, n, _, _, cs = lock
        return K, m, cs[0].shape[0]                # (after upload_lockstep_shared_ub_eq / _ub_tall: the structural costs only)

    def update_lockstep_vectors(self, bs=None, cs=None, c0s=None):
        """New b, c and c0 for every member of the resident lockstep batch (lpipm_update_lockstep_vectors), in the form of the
        upload_lockstep* that made it; None leaves those vectors (or constants) as they are.  A stays, and so does the first
        iteration's factor kept with it: the next solve_lockstep is bit-identical to a fresh upload of the same members."""
        K, m, nc = self._lockstep_form()
        bs = None if bs is None else [_f64(b) for b in bs]
        cs = None if cs is None else [_f64(c) for c in cs]
        if ((bs is not None and (len(bs) != K or any(b.shape != (m,) for b in bs)))
                or (cs is not None and (len(cs) != K or any(c.shape != (nc,) for c in cs)))
                or (c0s is not None and len(c0s) != K)):
            raise IncompatibleInputDimensions()
        dp = C.POINTER(C.c_double)
        arr = lambda lst: None if lst is None else (dp * K)(*[_p(a) for a in lst])
        c0 = (C.c_double * K)(*[float(v) for v in c0s]) if c0s is not None else None
        _raise_for(_capi.lib().lpipm_update_lockstep_vectors(self._h, K, arr(bs), arr(cs), c0))
        return self

    def update_lockstep_vectors_device(self, b_ptr, ldb, c_ptr, ldc, c0s=None):
        """update_lockstep_vectors from packed row blocks already on the device (lpipm_update_lockstep_vectors_device):
        member i's b at b_ptr + i * ldb doubles, its c at c_ptr + i * ldc; a null (0 / None) pointer leaves those vectors.
        The blocks are read on the context's stream: whatever wrote them must have completed."""
        K = self._lockstep_form()[0]
        if c0s is not None and len(c0s) != K:
            raise IncompatibleInputDimensions()
        c0 = (C.c_double * K)(*[float(v) for v in c0s]) if c0s is not None else None
        _raise_for(_capi.lib().lpipm_update_lockstep_vectors_device(
            self._h, K, C.c_void_p(int(b_ptr)) if b_ptr else None, int(ldb), C.c_void_p(int(c_ptr)) if c_ptr else None,
            int(ldc), c0))
        return self

    def set_first_factor_cache(self, on: bool = True):
        """Whether the first iteration's factor (a function of A alone) is kept per upload and reused by every later solve
        on it (lpipm_set_first_factor_cache; default on).  Off gives its memory back at the next upload."""
        _raise_for(_capi.lib().lpipm_set_first_factor_cache(self._h, int(bool(on))))
        return self

    def set_scaling(self, passes: int = 8):
        """Power-of-two row and column equilibration of every later upload on this context (lpipm_set_scaling): `passes`
        passes (1..64), 0 = off (the default).  Solutions come back in the caller's units; the iteration log and `tol` refer
        to the scaled problem."""
        _raise_for(_capi.lib().lpipm_set_scaling(self._h, int(passes)))
        return self

    def scaling(self, member: int = 0):
        """-> (row_exp, col_exp): the int32 exponents in use for resident member `member` (lpipm_get_scaling; one set for a
        single LP and for a shared-matrix batch).  All zero when scaling is off."""
        kr, kc = np.zeros(self.m, dtype=np.int32), np.zeros(self.n, dtype=np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        _raise_for(_capi.lib().lpipm_get_scaling(self._h, int(member), ip(kr), ip(kc)))
        return kr, kc

    def set_collective(self, rank: int, world: int, collective):
        """`collective.cfn` is an lpipm_allreduce_fn thunk (lp_amd.colsplit.TorchCollective); kept alive here."""
        self._collective = collective
        cfn = C.cast(collective.cfn, C.c_void_p) if collective is not None else None
        _raise_for(_capi.lib().lpipm_set_collective(self._h, int(rank), int(world), cfn, None))
        _raise_for(_capi.lib().lpipm_set_collective_on_stream(self._h, int(bool(getattr(collective, "on_stream", False)))))
        return self

    def upload_column_block(self, A_local, b, c_local, n_total: int, c0=0.0):
        """This rank's columns of one LP split over ranks (lpipm_upload_nsplit); solve_raw then returns
        this rank's slice of x."""
        A, b, c = _f64(A_local), _f64(b), _f64(c_local)
        if A.ndim != 2 or b.shape != (A.shape[0],) or c.shape != (A.shape[1],):
            raise IncompatibleInputDimensions()
        m, nl = A.shape
        _raise_for(_capi.lib().lpipm_upload_nsplit(self._h, m, int(n_total), nl, _p(A), nl, _p(b), _p(c), float(c0)))
        self.m, self.n, self._m_eq, self._members = m, nl, 0, 1
        return self

    def _upload_members(self, entry, head, bs, cs, c0s, m, n, nc, matrix, tail=()):
        """What the upload_lockstep* methods share: every member's b of m and c of nc entries checked, the pointer arrays and
        c0 made, `entry(ctx, K, *head, bs, cs, c0, *tail)` called and the resident batch (solutions of n entries) recorded."""
        K = len(bs)
        if K < 1 or len(cs) != K or any(b.shape != (m,) for b in bs) or any(c.shape != (nc,) for c in cs):
            raise IncompatibleInputDimensions()
        c0 = (C.c_double * K)(*[float(v) for v in c0s]) if c0s is not None else None
        _raise_for(getattr(_capi.lib(), entry)(self._h, K, *head, _ptrs(bs), _ptrs(cs), c0, *tail))
        self._lock = (K, m, n, matrix, bs, cs)      # keep the host arrays alive only for the duration of the call chain
        self.m, self.n, self._m_eq, self._members = m, n, 0, K
        return self

    def upload_lockstep(self, As, bs, cs, c0s=None, n_slack=0):
        """`len(As)` LPs of one shape resident at once (lpipm_upload_lockstep); solve with solve_lockstep.
        n_slack > 0 (lpipm_upload_lockstep_slack): the last n_slack columns of every member are the slack block [I; 0] of its
        `ub` rows, verified and then neither stored nor multiplied -- every member bit-identical to upload_arrays(..., n_slack)
        + solve_raw of that member alone."""
        As = [_f64(A) for A in As]; bs = [_f64(b) for b in bs]; cs = [_f64(c) for c in cs]
        if len(As) < 1 or len(bs) != len(As) or len(cs) != len(As):
            raise IncompatibleInputDimensions()
        m, n = As[0].shape
        if any(A.shape != (m, n) for A in As):
            raise IncompatibleInputDimensions()
        entry, tail = ("lpipm_upload_lockstep_slack", (int(n_slack),)) if n_slack else ("lpipm_upload_lockstep", ())
        return self._upload_members(entry, (m, n, _ptrs(As)), bs, cs, c0s, m, n, n, As, tail)

    def upload_lockstep_shared(self, A, bs, cs, c0s=None, n_slack=0):
        """`len(bs)` LPs that share ONE constraint matrix A, resident at once (lpipm_upload_lockstep_shared): member i is
        (A, bs[i], cs[i], c0s[i]).  A is held once on the device and each pass over it serves the whole batch; solve with
        solve_lockstep / solve_lockstep_device -- every member bit-identical to solving it alone.
        n_slack > 0 (lpipm_upload_lockstep_shared_slack): the last n_slack columns of A are its slack block [I; 0], verified
        and then neither stored nor multiplied, as upload_arrays(..., n_slack) does for one LP."""
        A = _f64(A); bs = [_f64(b) for b in bs]; cs = [_f64(c) for c in cs]
        if A.ndim != 2 or len(bs) < 1 or len(cs) != len(bs) or (c0s is not None and len(c0s) != len(bs)):
            raise IncompatibleInputDimensions()
        m, n = A.shape
        entry, tail = ("lpipm_upload_lockstep_shared_slack", (int(n_slack),)) if n_slack else ("lpipm_upload_lockstep_shared", ())
        return self._upload_members(entry, (m, n, _p(A), n), bs, cs, c0s, m, n, n, A, tail)

    def upload_lockstep_shared_ub_eq(self, A_ub, A_eq, bs, cs, c0s=None):
        """`len(bs)` inequality-form LPs over ONE pair of blocks (lpipm_upload_lockstep_shared_ub_eq): member i is
        min cs[i]'x st A_ub x <= bs[i][:m_ub], A_eq x == bs[i][m_ub:], x >= 0.  Either block may be None.  The blocks go to
        the device once, as they are; the slack block is never formed.  solve_lockstep then returns x with n + m_ub entries,
        slack values last -- every member bit-identical to Context.upload(Problem...ub().eq().build()) + solve_raw."""
        bs = [_f64(b) for b in bs]; cs = [_f64(c) for c in cs]
        if len(bs) < 1 or len(cs) != len(bs) or (c0s is not None and len(c0s) != len(bs)) or cs[0].ndim != 1:
            raise IncompatibleInputDimensions()
        n = cs[0].shape[0]
        A_ub = _f64(A_ub) if A_ub is not None else np.zeros((0, n))
        A_eq = _f64(A_eq) if A_eq is not None else np.zeros((0, n))
        if A_ub.ndim != 2 or A_eq.ndim != 2 or A_ub.shape[1] != n or A_eq.shape[1] != n:
            raise IncompatibleInputDimensions()
        m_ub, m_eq = A_ub.shape[0], A_eq.shape[0]
        head = (n, m_ub, _p(A_ub) if m_ub else None, n, m_eq, _p(A_eq) if m_eq else None, n)
        return self._upload_members("lpipm_upload_lockstep_shared_ub_eq", head, bs, cs, c0s, m_ub + m_eq, n + m_ub, n, None)

    def upload_lockstep_shared_ub_tall(self, A_ub, bs, cs, c0s=None):
        """`len(bs)` tall inequality-form LPs over ONE matrix (lpipm_upload_lockstep_shared_ub_tall): member i is
        min cs[i]'x st A_ub x <= bs[i], x >= 0, usually with many more rows than columns.  A_ub and its transpose are resident
        once; every member factors its own n x n reduced system.  solve_lockstep returns x with n + m_ub entries, slack values
        last -- every member bit-identical to Context.upload(Problem...ub().build(), tall=True) + solve_raw."""
        bs = [_f64(b) for b in bs]; cs = [_f64(c) for c in cs]
        if len(bs) < 1 or len(cs) != len(bs) or (c0s is not None and len(c0s) != len(bs)) or cs[0].ndim != 1:
            raise IncompatibleInputDimensions()
        n = cs[0].shape[0]
        A_ub = _f64(A_ub)
        if A_ub.ndim != 2 or A_ub.shape[1] != n:
            raise IncompatibleInputDimensions()
        m_ub = A_ub.shape[0]          # (the lockstep form: b[i] of m_ub, c[i] of the n structural costs)
        head = (n, m_ub, _p(A_ub) if m_ub else None, n)
        return self._upload_members("lpipm_upload_lockstep_shared_ub_tall", head, bs, cs, c0s, m_ub, n + m_ub, n, None)

    def upload_lockstep_shared_ub_eq_tall(self, A_ub, A_eq, bs, cs, c0s=None):
        """`len(bs)` tall LPs with equality rows over ONE pair of blocks (lpipm_upload_lockstep_shared_ub_eq_tall): member i is
        min cs[i]'x st A_ub x <= bs[i][:m_ub], A_eq x == bs[i][m_ub:], x >= 0, with many more `ub` rows than columns and a few
        `eq` rows.  The image [A_ub; A_eq] and the transpose of A_ub are resident once; every member factors its own n x n
        reduced system and its own m_eq x m_eq Schur complement.  A_eq None (or without rows): upload_lockstep_shared_ub_tall
        itself.  solve_lockstep returns x with n + m_ub entries, slack values last -- every member bit-identical to
        Context.upload_tall_eq(Problem...ub().eq().build()) + solve_raw."""
        bs = [_f64(b) for b in bs]; cs = [_f64(c) for c in cs]
        if len(bs) < 1 or len(cs) != len(bs) or (c0s is not None and len(c0s) != len(bs)) or cs[0].ndim != 1:
            raise IncompatibleInputDimensions()
        n = cs[0].shape[0]
        A_ub = _f64(A_ub) if A_ub is not None else np.zeros((0, n))
        A_eq = _f64(A_eq) if A_eq is not None else np.zeros((0, n))
        if A_ub.ndim != 2 or A_eq.ndim != 2 or A_ub.shape[1] != n or A_eq.shape[1] != n:
            raise IncompatibleInputDimensions()
        m_ub, m_eq = A_ub.shape[0], A_eq.shape[0]
        head = (n, m_ub, _p(A_ub) if m_ub else None, n, m_eq, _p(A_eq) if m_eq else None, n)
        return self._upload_members("lpipm_upload_lockstep_shared_ub_eq_tall", head, bs, cs, c0s, m_ub + m_eq, n + m_ub, n, None)

    def upload_lockstep_ub_tall(self, A_ubs, bs, cs, c0s=None):
        """`len(A_ubs)` independent tall inequality-form LPs of one shape, each with its own matrix
        (lpipm_upload_lockstep_ub_tall): member i is min cs[i]'x st A_ubs[i] x <= bs[i], x >= 0.  Every member keeps its own
        matrix, transpose and n x n reduced system on the device.  solve_lockstep returns x with n + m_ub entries, slack
        values last -- every member bit-identical to Context.upload(Problem...ub().build(), tall=True) + solve_raw."""
        A_ubs = [_f64(A) for A in A_ubs]; bs = [_f64(b) for b in bs]; cs = [_f64(c) for c in cs]
        if (len(A_ubs) < 1 or len(bs) != len(A_ubs) or len(cs) != len(A_ubs) or (c0s is not None and len(c0s) != len(A_ubs))
                or A_ubs[0].ndim != 2 or any(A.shape != A_ubs[0].shape for A in A_ubs)):
            raise IncompatibleInputDimensions()
        m_ub, n = A_ubs[0].shape
        head = (n, m_ub, _ptrs(A_ubs), n)
        return self._upload_members("lpipm_upload_lockstep_ub_tall", head, bs, cs, c0s, m_ub, n + m_ub, n, A_ubs)

    def resident_bytes(self) -> int:
        """Device bytes held for the resident problem(s): arenas + shared matrix + factor workspace."""
        out = C.c_uint64(0)
        _raise_for(_capi.lib().lpipm_get_resident_bytes(self._h, C.byref(out)))
        return int(out.value)

    def solve_lockstep(self, opts: "_capi.Opts"):
        """-> list of (status, x_slack | None, fun, iterations), one per LP of the last upload_lockstep"""
        K, m, n = self._lock[:3]
        xs = [np.full(n, np.nan) for _ in range(K)]
        out, unpack = _members_out(K, xs)
        return unpack(_capi.lib().lpipm_solve_lockstep(self._h, C.byref(opts), _ptrs(xs), *out))

    def solve_lockstep_device(self, opts: "_capi.Opts", x_dev_ptr: int, row_stride: int):
        """Like solve_lockstep, the solutions left in HBM: x / tau of LP i goes to the device row
        x_dev_ptr + i * row_stride doubles (lpipm_solve_lockstep_device).  -> list of (status, fun | None, iterations)"""
        out, unpack = _members_out(self._lock[0])
        return unpack(_capi.lib().lpipm_solve_lockstep_device(self._h, C.byref(opts), C.c_void_p(int(x_dev_ptr)), int(row_stride), *out))

    def solve_batch_device(self, problems, opts: "_capi.Opts", x_dev_ptr: int, row_stride: int, tall: bool = False):
        """lpipm_solve_batch_device over [(A, b, c, c0), ...]: member i's x / tau goes to the device row
        x_dev_ptr + i * row_stride doubles.  A fifth tuple element is the member's n_slack hint (lpipm_solve_batch_slack).
        tall=True: `problems` are Problems built from `ub` rows only (else ValueError), solved in the tall inequality form
        (lpipm_solve_batch_ub_tall); member i's row has n + m_ub entries, slack values last.
        -> list of (status, fun | None, iterations)"""
        return _solve_batch(self, problems, opts, tall, x_dev_ptr, row_stride)

    def solve_batch(self, problems, opts: "_capi.Opts", tall: bool = False):
        """lpipm_solve_batch over [(A, b, c, c0), ...] (any mix of shapes; equal shapes run as lockstep batches).
        A fifth tuple element is the member's n_slack hint (lpipm_solve_batch_slack): its slack block stays structural.
        tall=True: `problems` are Problems built from `ub` rows only (else ValueError), solved in the tall inequality form
        (lpipm_solve_batch_ub_tall: equal shapes as lockstep batches whose members own their matrices); x_slack has
        n + m_ub entries, slack values last.
        -> list of (status, x_slack | None, fun | None, iterations)"""
        return _solve_batch(self, problems, opts, tall)

    def solve_raw(self, opts: "_capi.Opts", want_log: bool = False, x_dev_ptr: int | None = None):
        """-> (status, x_slack | None, fun, iterations, log rows)"""
        x = None if x_dev_ptr is not None else np.full(self.n, np.nan)
        fun, it = C.c_double(np.nan), C.c_uint64(0)
        if want_log and opts.max_iter > (1 << 20):      # the library writes one row per iteration, up to max_iter of them
            raise InvalidParameter("want_log with max_iter > 2^20")
        nlog = int(opts.max_iter) if want_log else 0
        log = (_capi.IterRow * max(nlog, 1))() if want_log else None
        if x_dev_ptr is not None:
            rc = _capi.lib().lpipm_solve_device(self._h, C.byref(opts), C.c_void_p(int(x_dev_ptr)), C.byref(fun),
                                                C.byref(it), log)
        else:
            rc = _capi.lib().lpipm_solve(self._h, C.byref(opts), _p(x), C.byref(fun), C.byref(it), log)
        rows = []
        if want_log:
            for i in range(min(int(it.value), nlog)):
                r = log[i]
                rows.append((r.alpha, r.rho_p, r.rho_d, r.rho_A, r.rho_g, r.rho_mu, r.obj))
        return rc, x, fun.value, int(it.value), rows

    def _duals_lengths(self):
        """(members, len(y), len(z)) of what is resident, as the uploads recorded them; BackendError when nothing is (before an
        upload, after solve_batch*): the getter's buffers are never sized for another problem than the one C holds."""
        if self._members < 1 or self.m < 1 or self.n < 1:
            raise BackendError("no resident problem on this context: upload and solve before asking for duals")
        return self._members, self.m, self.n

    def duals(self, member: int = 0) -> dict:
        """The duals of resident member `member` (0 for a single LP) at the iterate of the LAST solve on this context
        (lpipm_get_duals): dict(y, z, dual_fun, tau, kappa) -- y the multipliers of the upload's rows, z the reduced costs, as
        long as x_slack, both in the caller's units; A'y + z = c, z >= 0, d fun / d b_i = y_i.  A member without a solution
        raises its LinearProgramError subclass; a context without a completed solve raises BackendError."""
        _, m, n = self._duals_lengths()
        y, z = np.full(m, np.nan), np.full(n, np.nan)
        info = _capi.DualInfo()
        _raise_for(_capi.lib().lpipm_get_duals(self._h, int(member), _p(y), _p(z), C.byref(info)))
        return dict(y=y, z=z, dual_fun=info.dual_fun, tau=info.tau, kappa=info.kappa)

    def _get_duals_device(self, y_ptr, ldy, z_ptr, ldz):
        """lpipm_get_duals_device -> the lpipm_dual_info records, one per resident member."""
        info = (_capi.DualInfo * self._duals_lengths()[0])()
        _raise_for(_capi.lib().lpipm_get_duals_device(self._h, C.c_void_p(int(y_ptr)) if y_ptr else None, int(ldy),
                                                      C.c_void_p(int(z_ptr)) if z_ptr else None, int(ldz), info))
        return info

    def duals_lockstep(self, members: int | None = None) -> list:
        """Context.duals of the first `members` (default: all) members of the resident lockstep batch after its
        solve_lockstep[_device]: a list of that dict, None for a member without a solution.  One lpipm_get_duals_device into
        one device block and one copy of that block to the host, whatever the count: the same bits as one lpipm_get_duals per
        member."""
        import torch
        K, m, n = self._duals_lengths()
        block = torch.empty((K, m + n), dtype=torch.float64, device=torch.device("cuda", self.device))
        torch.cuda.current_stream(self.device).synchronize()      # (the block may be recycled memory torch still works on)
        info = self._get_duals_device(block.data_ptr(), m + n, block.data_ptr() + 8 * m, m + n)
        keep = K if members is None else min(int(members), K)
        rows = block[:keep].cpu().numpy()
        return [dict(y=rows[k, :m].copy(), z=rows[k, m:].copy(), dual_fun=info[k].dual_fun, tau=info[k].tau, kappa=info[k].kappa)
                if has_x(info[k].status) else None for k in range(keep)]

    def duals_device(self, y_ptr, ldy: int, z_ptr, ldz: int) -> list:
        """The duals of every resident member left in HBM (lpipm_get_duals_device): member i's y to the device row
        y_ptr + i * ldy doubles, its z to z_ptr + i * ldz; a null (0 / None) pointer skips those vectors, the rows of a member
        without a solution stay untouched.  Complete on return.  -> list of (status, dual_fun | None)"""
        return [(r.status, r.dual_fun if has_x(r.status) else None) for r in self._get_duals_device(y_ptr, ldy, z_ptr, ldz)]

    @staticmethod
    def _certificate_dict(info, y, col):
        kind = int(info.kind)
        return dict(kind=kind, status=int(info.status), y=y if kind == _capi.CERT_FARKAS else None,
                    col=col if kind != _capi.CERT_NONE else None, scale=info.scale, residual=info.residual, tau=info.tau,
                    kappa=info.kappa)

    def certificate(self, member: int = 0) -> dict:
        """The certificate of resident member `member` (0 for a single LP) at the iterate of the LAST solve on this context
        (lpipm_get_certificate): dict(kind, status, y, col, scale, residual, tau, kappa).  kind 1 (status Infeasible): the
        Farkas ray y, col = z with A'y + z ~ 0, z >= 0, b.y = 1; kind 2 (status Unbounded, c.x < 0): col = x with A x ~ 0,
        x >= 0, c.x = -1, y None; kind 0 (any other status, or an Unbounded call that proves nothing): y and col None.  In the
        caller's units; residual is max|A'y + z|, respectively max|A x|.  A context without a completed solve raises
        BackendError."""
        _, m, n = self._duals_lengths()
        y, col = np.full(m, np.nan), np.full(n, np.nan)
        info = _capi.CertInfo()
        _raise_for(_capi.lib().lpipm_get_certificate(self._h, int(member), _p(y), _p(col), C.byref(info)))
        return self._certificate_dict(info, y, col)

    def _get_certificates_device(self, y_ptr, ldy, col_ptr, ldc):
        """lpipm_get_certificate_device -> the lpipm_cert_info records, one per resident member."""
        info = (_capi.CertInfo * self._duals_lengths()[0])()
        _raise_for(_capi.lib().lpipm_get_certificate_device(self._h, C.c_void_p(int(y_ptr)) if y_ptr else None, int(ldy),
                                                            C.c_void_p(int(col_ptr)) if col_ptr else None, int(ldc), info))
        return info

    def certificates_lockstep(self, members: int | None = None) -> list:
        """Context.certificate of the first `members` (default: all) members of the resident lockstep batch after its
        solve_lockstep[_device]: a list of that dict.  One lpipm_get_certificate_device into one device block and one copy
        of that block to the host, whatever the count: the same bits as one lpipm_get_certificate per member."""
        import torch
        K, m, n = self._duals_lengths()
        block = torch.empty((K, m + n), dtype=torch.float64, device=torch.device("cuda", self.device))
        torch.cuda.current_stream(self.device).synchronize()      # (the block may be recycled memory torch still works on)
        info = self._get_certificates_device(block.data_ptr(), m + n, block.data_ptr() + 8 * m, m + n)
        keep = K if members is None else min(int(members), K)
        rows = block[:keep].cpu().numpy()
        return [self._certificate_dict(info[k], rows[k, :m].copy(), rows[k, m:].copy()) for k in range(keep)]

    def certificates_device(self, y_ptr, ldy: int, col_ptr, ldc: int) -> list:
        """The certificates of every resident member left in HBM (lpipm_get_certificate_device): member i's Farkas y to the
        device row y_ptr + i * ldy doubles, its z or x to col_ptr + i * ldc; a null (0 / None) pointer skips those vectors,
        the rows of a member without a certificate stay untouched.  Complete on return.
        -> list of dict(kind, status, scale, residual, tau, kappa)"""
        return [dict(kind=int(r.kind), status=int(r.status), scale=r.scale, residual=r.residual, tau=r.tau, kappa=r.kappa)
                for r in self._get_certificates_device(y_ptr, ldy, col_ptr, ldc)]

    def solve_f32(self, A, b, c, c0: float = 0.0, opts: "_capi.Opts | None" = None, want_log: bool = False):
        """InteriorPoint<f32>::solve on a slack-form problem (src/float.rs:42-43; lpipm_solve_f32): every operation in f32.
        -> (status, x_slack float32 | None, fun, iterations, log rows).  The context's uploaded fp64 problem, if any, is untouched."""
        A = np.ascontiguousarray(A, dtype=np.float32); b = np.ascontiguousarray(b, dtype=np.float32)
        c = np.ascontiguousarray(c, dtype=np.float32)
        if A.ndim != 2 or b.shape != (A.shape[0],) or c.shape != (A.shape[1],):
            raise IncompatibleInputDimensions()
        opts = opts or InteriorPoint.default().opts()
        m, n = A.shape
        x = np.full(n, np.nan, dtype=np.float32)
        fun, it = C.c_float(np.nan), C.c_uint64(0)
        nlog = int(opts.max_iter) if want_log else 0
        log = (C.c_float * (7 * max(nlog, 1)))() if want_log else None
        fp = lambda a_: a_.ctypes.data_as(C.POINTER(C.c_float))
        rc = _capi.lib().lpipm_solve_f32(self._h, m, n, fp(A), n, fp(b), fp(c), C.c_float(c0), C.byref(opts), fp(x), C.byref(fun),
                                         C.byref(it), C.cast(log, C.c_void_p) if want_log else None)
        rows = [tuple(float(log[7 * i + k]) for k in range(7)) for i in range(min(int(it.value), nlog))] if want_log else []
        return rc, (x if has_x(rc) else None), float(fun.value), int(it.value), rows

    def k_generic_solve_f64(self, A, b, c, c0: float = 0.0, opts: "_capi.Opts | None" = None, want_log: bool = False):
        """Test hook: the generic (scalar-type-templated) kernels of the f32 instantiation, instantiated for double."""
        A, b, c = _f64(A), _f64(b), _f64(c)
        opts = opts or InteriorPoint.default().opts()
        m, n = A.shape
        x = np.full(n, np.nan)
        fun, it = C.c_double(np.nan), C.c_uint64(0)
        nlog = int(opts.max_iter) if want_log else 0
        log = (_capi.IterRow * max(nlog, 1))() if want_log else None
        rc = _capi.lib().lpipm_k_generic_solve_f64(self._h, m, n, _p(A), n, _p(b), _p(c), C.c_double(c0), C.byref(opts), _p(x),
                                                   C.byref(fun), C.byref(it), C.cast(log, C.c_void_p) if want_log else None)
        rows = [(r.alpha, r.rho_p, r.rho_d, r.rho_A, r.rho_g, r.rho_mu, r.obj) for r in list(log)[:min(int(it.value), nlog)]] if want_log else []
        return rc, x, fun.value, int(it.value), rows

    def set_profiling(self, on):
        """False/0 off, True/1 every phase, 2 only the A.D.A^T launches (2 events per iteration)."""
        _capi.lib().lpipm_set_profiling(self._h, int(on))

    def phase_times(self) -> dict:
        t = _capi.PhaseTimes()
        _capi.lib().lpipm_get_phase_times(self._h, C.byref(t))
        return {k: getattr(t, k) for k, _ in _capi.PhaseTimes._fields_}

    # ---- kernel-granularity entry points (parity tests / micro-benchmarks).  The C entries read what the resident shape or
    # the given m says, so every array is checked against that first: a wrong shape is IncompatibleInputDimensions, and no
    # entry is handed a buffer shorter than it reads.
    def _need_problem(self):
        """Raises what every entry raises without a resident problem (self.m and self.n mean nothing then)."""
        _raise_for(_capi.lib().lpipm_k_resident_matrix(self._h, 0, 0, 0, None, 0, None, None))

    def k_adat(self, dinv, repeats=1):
        self._need_problem()
        dinv = _vec(dinv, self.n)
        M = np.empty((self.m, self.m))
        ms = C.c_double(0)
        _raise_for(_capi.lib().lpipm_k_adat(self._h, _p(dinv), _p(M), repeats, C.byref(ms)))
        return M, ms.value

    def k_tall_normal(self, dinv):
        """K = X^T diag(1/dinv_s) X + diag(1/dinv_x) of the tall upload (lower triangle valid)."""
        dinv = _f64(dinv)
        if dinv.shape != (self.n,):
            raise IncompatibleInputDimensions()
        nx = self.n - (self.m - self._m_eq)
        K = np.empty((nx, nx))
        _raise_for(_capi.lib().lpipm_k_tall_normal(self._h, _p(dinv), _p(K)))
        return K

    def k_tall_schur(self, dinv):
        """S = A_eq K^-1 A_eq^T of the upload_tall_eq problem at dinv (m_eq x m_eq, lower triangle valid), as built from
        Zt = A_eq L^-T behind K's factorisation."""
        dinv = _f64(dinv)
        if dinv.shape != (self.n,):
            raise IncompatibleInputDimensions()
        S = np.empty((self._m_eq, self._m_eq))
        _raise_for(_capi.lib().lpipm_k_tall_schur(self._h, _p(dinv), _p(S)))
        return S

    def k_tall_sym_solve(self, dinv, R1, R2):
        """The reduced sym_solve of the tall upload at dinv for 1 or 2 right-hand sides: R1 (nrhs, n), R2 (nrhs, m)
        -> U (nrhs, n), V (nrhs, m), info."""
        dinv = _f64(dinv)
        R1, R2 = np.atleast_2d(_f64(R1)), np.atleast_2d(_f64(R2))
        nrhs = R1.shape[0]
        if dinv.shape != (self.n,) or R1.shape != (nrhs, self.n) or R2.shape != (nrhs, self.m):
            raise IncompatibleInputDimensions()
        U, V = np.empty((nrhs, self.n)), np.empty((nrhs, self.m))
        info = C.c_int32(0)
        _raise_for(_capi.lib().lpipm_k_tall_sym_solve(self._h, _p(dinv), nrhs, _p(R1), _p(R2), _p(U), _p(V), C.byref(info)))
        return U, V, info.value

    def k_bounded_normal(self, dinv_ext, m: int):
        """M~ = A diag(D~) A^T (+ D~ of the `ub` slacks on their rows) of the bounded upload at dinv_ext, the x / z of all
        n + nb columns: m x m, m the rows WITHOUT the bound rows, lower triangle valid."""
        dinv_ext = _f64(dinv_ext)
        if dinv_ext.shape != (self.n,):
            raise IncompatibleInputDimensions()
        M = np.empty((int(m), int(m)))
        _raise_for(_capi.lib().lpipm_k_bounded_normal(self._h, _p(dinv_ext), _p(M)))
        return M

    def k_bounded_sym_solve(self, dinv_ext, R1, R2):
        """The reduced sym_solve of the bounded upload at dinv_ext for 1 or 2 right-hand sides of the explicit LP: R1
        (nrhs, n), R2 (nrhs, m), n and m the extended lengths -> U (nrhs, n), V (nrhs, m), info."""
        dinv_ext = _f64(dinv_ext)
        R1, R2 = np.atleast_2d(_f64(R1)), np.atleast_2d(_f64(R2))
        nrhs = R1.shape[0]
        if dinv_ext.shape != (self.n,) or R1.shape != (nrhs, self.n) or R2.shape != (nrhs, self.m):
            raise IncompatibleInputDimensions()
        U, V = np.empty((nrhs, self.n)), np.empty((nrhs, self.m))
        info = C.c_int32(0)
        _raise_for(_capi.lib().lpipm_k_bounded_sym_solve(self._h, _p(dinv_ext), nrhs, _p(R1), _p(R2), _p(U), _p(V), C.byref(info)))
        return U, V, info.value

    def k_potrf(self, M, repeats=1):
        L = _square(M).copy()
        info, ms = C.c_int32(0), C.c_double(0)
        _raise_for(_capi.lib().lpipm_k_potrf(self._h, L.shape[0], _p(L), C.byref(info), repeats, C.byref(ms)))
        return L, info.value, ms.value

    def k_factor_inverses(self, m):
        """After k_potrf at size m: (inv, invT, super-block width).  inv / invT are mp x mp (mp = m rounded up to 128), zero but
        for the diagonal super-blocks, which hold inv(L_ss) and inv(L_ss)^T as the solves read them."""
        mp = -(-int(m) // 128) * 128
        inv, invT = np.empty((mp, mp)), np.empty((mp, mp))
        w = C.c_int32(0)
        _raise_for(_capi.lib().lpipm_k_factor_inverses(self._h, m, _p(inv), _p(invT), C.byref(w)))
        return inv, invT, w.value

    def k_potrf_lockstep(self, Ms):
        """The factors and info words of `count` m x m matrices factored as ONE lockstep batch."""
        L = _f64(Ms).copy()
        if L.ndim != 3 or L.shape[1] != L.shape[2]:
            raise IncompatibleInputDimensions()
        count, m = L.shape[0], L.shape[1]
        infos = np.zeros(count, dtype=np.int32)
        _raise_for(_capi.lib().lpipm_k_potrf_lockstep(self._h, m, count, _p(L), infos.ctypes.data_as(C.POINTER(C.c_int32))))
        return L, infos

    def k_trsm_lt_lockstep(self, Ms, B, done_mask=None, fill=0.0):
        """Z = B L^-T for every member of a lockstep batch (lpipm_k_trsm_lt_lockstep): Ms (count, n, n) SPD, factored as one
        batch; B (rows, cols) is one block for all members, B (count, rows, cols) one per member.  -> (Z, infos) with Z
        (count, round_up(rows, 16), round_up(n, 128)).  Every Z starts as `fill`; a member whose done_mask entry is non-zero is
        skipped and keeps it."""
        Ms = np.ascontiguousarray(_f64(Ms)); B = np.ascontiguousarray(_f64(B))
        if Ms.ndim != 3 or Ms.shape[1] != Ms.shape[2] or B.ndim not in (2, 3):
            raise IncompatibleInputDimensions()
        count, n = Ms.shape[0], Ms.shape[1]
        shared = B.ndim == 2
        rows, cols = B.shape[-2:]
        if (not shared and B.shape[0] != count) or cols > n or rows < 1 or cols < 1:
            raise IncompatibleInputDimensions()
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        mask = None
        if done_mask is not None:
            mask = np.ascontiguousarray(done_mask, dtype=np.int32)
            if mask.shape != (count,):
                raise IncompatibleInputDimensions()
        Z = np.full((count, -(-rows // 16) * 16, -(-n // 128) * 128), float(fill))
        infos = np.zeros(count, dtype=np.int32)
        _raise_for(_capi.lib().lpipm_k_trsm_lt_lockstep(self._h, n, count, rows, cols, int(shared), _p(Ms), _p(B), cols, _p(Z), ip(infos),
                                                        ip(mask) if mask is not None else None))
        return Z, infos

    def k_chol_solve(self, m, R, repeats=1):
        R = _rows(R, int(m))
        V = np.empty_like(R)
        ms = C.c_double(0)
        _raise_for(_capi.lib().lpipm_k_chol_solve(self._h, m, R.shape[0], _p(R), _p(V), repeats, C.byref(ms)))
        return V, ms.value

    def k_chol_solve_split(self, m, R, split):
        """k_chol_solve as two calls of the sweep: forward steps [0, split), then the rest."""
        R = _rows(R, int(m))
        V = np.empty_like(R)
        _raise_for(_capi.lib().lpipm_k_chol_solve_split(self._h, m, R.shape[0], _p(R), _p(V), split))
        return V

    def k_symv_residual(self, M, V, R0):
        M = _square(M); V = _rows(V, M.shape[0]); R0 = _rows(R0, M.shape[0])
        if R0.shape != V.shape:
            raise IncompatibleInputDimensions()
        Rho = np.empty_like(V)
        _raise_for(_capi.lib().lpipm_k_symv_residual(self._h, M.shape[0], _p(M), V.shape[0], _p(V), _p(R0), _p(Rho)))
        return Rho

    def k_qr_solve(self, M, R):
        M = _square(M)
        R = _rows(R, M.shape[0])
        V = np.empty_like(R)
        info, ms = C.c_int32(0), C.c_double(0)
        _raise_for(_capi.lib().lpipm_k_qr_solve(self._h, M.shape[0], _p(M), R.shape[0], _p(R), _p(V), C.byref(info),
                                                C.byref(ms)))
        return V, info.value, ms.value

    def k_gemv_n(self, W, repeats=1):
        self._need_problem()
        W = _rows(W, self.n)
        Y = np.empty((W.shape[0], self.m))
        ms = C.c_double(0)
        _raise_for(_capi.lib().lpipm_k_gemv_n(self._h, W.shape[0], _p(W), _p(Y), repeats, C.byref(ms)))
        return Y, ms.value

    def k_gemv_t(self, V, repeats=1):
        self._need_problem()
        V = _rows(V, self.m)
        U = np.empty((V.shape[0], self.n))
        ms = C.c_double(0)
        _raise_for(_capi.lib().lpipm_k_gemv_t(self._h, V.shape[0], _p(V), _p(U), repeats, C.byref(ms)))
        return U, ms.value

    def k_iteration(self, opts, x, y, z, tau, kappa, ip=False):
        """One loop body of solve_normal_form from the given iterate (lpipm_k_iteration).
        -> dict(x, y, z, tau, kappa, d_x, d_y, d_z, d_tau, d_kappa, alpha, info)"""
        self._need_problem()
        x, y, z = _vec(x, self.n).copy(), _vec(y, self.m).copy(), _vec(z, self.n).copy()
        tk = np.array([float(tau), float(kappa)])
        dx, dy, dz, dtk, al = np.empty(self.n), np.empty(self.m), np.empty(self.n), np.empty(2), np.empty(1)
        info = C.c_int32(0)
        _raise_for(_capi.lib().lpipm_k_iteration(self._h, C.byref(opts), int(bool(ip)), _p(x), _p(y), _p(z), _p(tk[0:1]),
                                                 _p(tk[1:2]), _p(dx), _p(dy), _p(dz), _p(dtk), _p(al), C.byref(info)))
        return dict(x=x, y=y, z=z, tau=float(tk[0]), kappa=float(tk[1]), d_x=dx, d_y=dy, d_z=dz, d_tau=float(dtk[0]),
                    d_kappa=float(dtk[1]), alpha=float(al[0]), info=info.value)

    def k_gemv_dual(self, w, v, repeats=1):
        self._need_problem()
        w, v = _vec(w, self.n), _vec(v, self.m)
        Aw, ATv = np.empty(self.m), np.empty(self.n)
        ms = C.c_double(0)
        _raise_for(_capi.lib().lpipm_k_gemv_dual(self._h, _p(w), _p(v), _p(Aw), _p(ATv), repeats, C.byref(ms)))
        return Aw, ATv, ms.value

    def k_mfma_f64_probe(self, iters=20000):
        tf, ms = C.c_double(0), C.c_double(0)
        _raise_for(_capi.lib().lpipm_k_mfma_f64_probe(self._h, iters, C.byref(tf), C.byref(ms)))
        return tf.value, ms.value


_default_ctx: dict[int, Context] = {}


def default_context(device: int = 0) -> Context:
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


# ------------------------------------------------------------------------------ interior_point/mod.rs
class InteriorPointBuilder:
    """interior_point/mod.rs:41-138."""

    def __init__(self):
        o = _capi.Opts()
        _capi.lib().lpipm_default_opts(C.byref(o))   # mod.rs:50-60
        self._tol, self._disp, self._ip = o.tol, bool(o.disp), bool(o.ip)
        self._solver_type, self._alpha0, self._max_iter = EquationSolverType(o.solver_type), o.alpha0, o.max_iter

    def tol(self, tol):
        self._tol = float(tol)
        return self

    def disp(self, disp):
        self._disp = bool(disp)
        return self

    def ip(self, ip):
        self._ip = bool(ip)
        return self

    def solver_type(self, solver_type):
        self._solver_type = EquationSolverType(solver_type)
        return self

    def alpha0(self, alpha0):
        self._alpha0 = float(alpha0)
        return self

    def max_iter(self, max_iter):
        self._max_iter = int(max_iter)
        return self

    def build(self) -> "InteriorPoint":           # mod.rs:118-137
        if self._alpha0 <= 0.0 or self._alpha0 >= 1.0:
            raise InvalidParameter("Alpha0 must be between 0 and 1 (exclusive)")
        if self._tol <= 0.0:
            raise InvalidParameter("The tolerance must be nonnegative.")
        return InteriorPoint(self._tol, self._disp, self._ip, self._solver_type, self._alpha0, self._max_iter)


class InteriorPoint(Solver):
    """interior_point/mod.rs:140-241.  `device` selects the GPU (no reference analogue; default 0)."""

    def __init__(self, tol, disp, ip, solver_type, alpha0, max_iter, device: int = 0):
        self._tol, self._disp, self._ip = tol, disp, ip
        self._solver_type, self._alpha0, self._max_iter = solver_type, alpha0, max_iter
        self.device = device

    @staticmethod
    def default() -> "InteriorPoint":             # mod.rs:154-159
        return InteriorPointBuilder().build()

    @staticmethod
    def custom() -> InteriorPointBuilder:         # mod.rs:195-197
        return InteriorPointBuilder()

    def __eq__(self, other):                      # derive(PartialEq), mod.rs:140
        return isinstance(other, InteriorPoint) and self._key() == other._key()

    def _key(self):
        return (self._tol, self._disp, self._ip, self._solver_type, self._alpha0, self._max_iter)

    def opts(self) -> "_capi.Opts":
        return _capi.Opts(self._tol, self._alpha0, self._max_iter, int(self._ip), int(self._solver_type),
                          int(self._disp))

    def solve(self, problem: Problem) -> OptimizeResult:     # mod.rs:161-168
        ctx = default_context(self.device)
        if problem.dtype == np.float32:                      # InteriorPoint<f32> (src/float.rs:42-43)
            rc, x_slack, fun, it, _ = ctx.solve_f32(problem.A(), problem.b(), problem.c(), problem.c0(), self.opts())
            if rc == _capi.ITERATION_LIMIT:
                raise IterationLimitExceeded(x_slack)
            _raise_for(rc)
            return OptimizeResult(problem.denormalize_x_into(x_slack), fun, it)
        ctx.upload(problem)
        return self.solve_uploaded(ctx, problem)

    def solve_uploaded(self, ctx: Context, problem: Problem, want_log=False, want_duals=False, want_certificate=False):
        """want_duals: the result also carries y_ub, y_eq, reduced_costs (Problem.denormalize_duals of Context.duals) and
        dual_fun of the solve's last iterate.  want_certificate: a raised Infeasible / Unbounded carries .certificate
        (solve_with_certificate)."""
        rc, x_slack, fun, it, rows = ctx.solve_raw(self.opts(), want_log=want_log)
        if rc == _capi.ITERATION_LIMIT:
            raise IterationLimitExceeded(x_slack)            # mod.rs:237-239 (payload: x / tau, slack form)
        if want_certificate and rc in (_capi.INFEASIBLE, _capi.UNBOUNDED):
            d = ctx.certificate()
            err = _BY_CODE[rc]()
            y_ub, y_eq, cut = problem.denormalize_certificate(d["y"], d["col"], d["kind"])
            err.certificate = dict(kind=d["kind"], y_ub=y_ub, y_eq=y_eq, z=cut if d["kind"] == _capi.CERT_FARKAS else None,
                                   x=cut if d["kind"] == _capi.CERT_RAY else None, scale=d["scale"], residual=d["residual"],
                                   tau=d["tau"], kappa=d["kappa"])
            if problem.n_bounded():
                err.certificate["y_upper"] = problem.denormalize_bound_certificate(d["y"], d["kind"])
            raise err
        _raise_for(rc)
        res = OptimizeResult(problem.denormalize_x_into(x_slack), fun, it)   # mod.rs:165-167
        if want_log:
            res.log = rows
            res.x_slack = x_slack
        if want_duals:
            d = ctx.duals()
            res.y_ub, res.y_eq, res.reduced_costs = problem.denormalize_duals(d["y"], d["z"])
            res.dual_fun = d["dual_fun"]
            res.upper = problem.denormalize_bound_duals(d["z"])
        return res

    def solve_with_duals(self, problem: Problem) -> OptimizeResult:
        """solve(problem) with the duals of its last iterate: the OptimizeResult plus y_ub, y_eq (the multipliers of the `ub`
        and `eq` rows, d fun / d b), reduced_costs (of the structural columns) and dual_fun.  (A Problem<f32> has none:
        lpipm_solve_f32 releases its problem inside the call.)"""
        if problem.dtype == np.float32:
            raise ValueError("solve_with_duals needs a float64 Problem")
        ctx = default_context(self.device)
        ctx.upload(problem)
        return self.solve_uploaded(ctx, problem, want_duals=True)

    def solve_with_certificate(self, problem: Problem) -> OptimizeResult:
        """solve(problem), but a raised Infeasible or Unbounded carries .certificate: dict(kind, y_ub, y_eq, z, x, scale,
        residual, tau, kappa) -- kind 1: the Farkas multipliers of the `ub` and `eq` rows and z of the structural columns
        (A_ub^T y_ub + A_eq^T y_eq + z ~ 0, y_ub <= 0, z >= 0, b.y = 1: a feasibility cut); kind 2: the improving ray x of the
        structural columns (A_ub x <= 0, A_eq x ~ 0, x >= 0, c.x = -1); kind 0: an Unbounded call that proves nothing.  The
        fields a kind does not have are None.  (A Problem<f32> has none: lpipm_solve_f32 releases its problem inside the call.)"""
        if problem.dtype == np.float32:
            raise ValueError("solve_with_certificate needs a float64 Problem")
        ctx = default_context(self.device)
        ctx.upload(problem)
        return self.solve_uploaded(ctx, problem, want_certificate=True)
