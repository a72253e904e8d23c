"""The inputs of the SVR solver's edge tests, shared by tests/test_svr_edges_ref_cpu.py (which asserts, on the restatement of
tests/svr_fit_ref.py alone, the conditions that make each input meaningful) and tests/test_svr_edges_gpu.py (which runs them
through svr_smo_kernel).  Plain NumPy; imports nothing from the package.

A solver task is what audioTrainTest.svr_solve takes: (rows, mean, scale, C, gamma, epsilon), the targets being y[rows] of the
call's target vector; a sweep job what svr_split_fit_predict takes: (train_idx, test_idx, mean, scale, C)."""
import collections
import functools

import numpy as np

import smo_edge_cases

# ---------------------------------------------------------------------------------------------------------------------
# (a) the trajectory set: tasks whose every selection is decided by a margin far above rounding, so that the path of a
#     correct solver is the restatement's, step by step
# ---------------------------------------------------------------------------------------------------------------------
N_RANDOM = 160
N_INTEGER = 8               # samples 160 + k = (k, 0, ..) with the target INT_TARGETS[k]; samples 168 + k and 176 + k: the same
INT_TARGETS = (0.0, 2.0, 1.0, 4.0, 3.0, 6.0, 5.0, 8.0)    # point again with the target moved by INT_COPY_SHIFTS: one point, three
INT_COPY_SHIFTS = (0.0, 3.0, -1.5)                         # targets, eta between their variables exactly 0
EQUAL0, N_EQUAL, EQUAL_TARGET = N_RANDOM + 3 * N_INTEGER, 8, 1.5       # samples that share one target
TUBE0, N_TUBE, TUBE_CENTRE, TUBE_HALF = EQUAL0 + N_EQUAL, 20, 2.0, 0.09   # targets within 0.09 of 2: inside a tube of 0.1
BOUND0, N_BOUND = TUBE0 + N_TUBE, 40                                    # targets near +5 and -5 in alternation
N_SAMPLES = BOUND0 + N_BOUND

Trajectory = collections.namedtuple("Trajectory", "name n_dims kernel eps task tau")
# (n_dims, kernel, rows, C, eps, seed, gamma (None: 1 / n_dims), epsilon): fixed seeds, found by a search over the restatement
# for tasks that meet the conditions of test_svr_edges_ref_cpu.py.  The first task of a batch key (n_dims, kernel, eps) is the
# one whose epsilon and gamma a kernel that read task 0's for every task would use.
TRAJECTORY_SPECS = (
    (1, "linear", 5, 1.0, 1e-2, 84, None, 0.0),
    (1, "linear", 70, 0.05, 1e-2, 45, None, 0.5),
    (1, "linear", 5, 0.05, 1e-2, 20, None, 0.1),
    (1, "linear", 16, 1.0, 1e-3, 69, None, 0.5),
    (1, "linear", 16, 0.05, 1e-3, 73, None, 0.5),
    (1, "rbf", 5, 20.0, 1e-1, 7, None, 0.0),
    (1, "rbf", 70, 1.0, 1e-1, 23, None, 0.5),
    (9, "linear", 47, 0.05, 1e-1, 31, None, 0.0),
    (9, "linear", 47, 0.05, 1e-1, 31, None, 0.1),          # the task above under another epsilon, in the same batch
    (9, "linear", 8, 0.05, 1e-1, 36, None, 0.0),
    (9, "linear", 12, 0.05, 1e-2, 77, None, 0.1),
    (9, "linear", 12, 0.05, 1e-2, 15, None, 0.5),
    (9, "rbf", 33, 1.0, 1e-2, 1, None, 0.1),
    (9, "rbf", 33, 1.0, 1e-2, 1, 0.05, 0.1),               # likewise under another gamma
    (9, "rbf", 33, 1.0, 1e-2, 1, None, 0.0),               # and under another epsilon
    (9, "rbf", 70, 0.05, 1e-3, 13, None, 0.0),
    (256, "linear", 2, 20.0, 1e-3, 48, None, 0.1),
    (256, "linear", 5, 1.0, 1e-1, 46, None, 0.0),
    (256, "rbf", 47, 0.05, 1e-2, 97, None, 0.0),
    (256, "rbf", 47, 0.05, 1e-2, 97, 2.5 / 256.0, 0.0),    # another gamma
    (256, "rbf", 2, 1.0, 1e-2, 8, None, 0.0),
)
# the TAU tasks: (n_dims, name, samples, C, epsilon) over the integer samples (sample s is the point s % 8, copy s // 8), mean
# 0 / scale 1, linear kernel, eps 1e-3.  Each holds the three copies of one point; the step that pairs two of them comes second or
# third on the path.  With TWO candidates at an eta of exactly 0 a solver that leaves eta = 0 in place ties b^2 / 0 = inf
# against inf where libsvm compares b^2 / TAU (with one, inf and b^2 / TAU win alike and both steps are clipped to the same
# bound): these tasks tell the two solvers apart.
TAU_SPECS = (
    (1, "tau5", (16, 3, 15, 0, 8), 20.0, 0.5),
    (9, "tau6", (18, 2, 20, 10, 21, 7), 1.0, 0.0),
    (256, "tau6", (22, 15, 17, 16, 9, 1), 0.05, 0.1),
)


@functools.lru_cache(maxsize=None)
def trajectory_matrix(n_dims):
    """(X [N_SAMPLES][n_dims], y [N_SAMPLES]): 160 Gaussian samples whose target is a smooth function of two directions plus
    noise (deviation about 1: rows outside a tube of 0.1 and of 0.5); the integer samples and their twins; the samples the
    degenerate tasks own.  Read-only."""
    rng = np.random.default_rng(900 + n_dims)
    w = rng.standard_normal((2, n_dims)) / np.sqrt(n_dims)
    spread, centre = rng.uniform(0.5, 2.0, n_dims), rng.normal(0, 2, n_dims)
    U = rng.standard_normal((N_SAMPLES, n_dims))
    y = 0.8 * (U @ w[0]) + 0.6 * np.tanh(U @ w[1]) + 0.3 * rng.standard_normal(N_SAMPLES)
    X = U * spread + centre
    ints = np.zeros((N_INTEGER, n_dims))
    ints[:, 0] = np.arange(N_INTEGER)
    for c, shift in enumerate(INT_COPY_SHIFTS):
        X[N_RANDOM + c * N_INTEGER:N_RANDOM + (c + 1) * N_INTEGER] = ints
        y[N_RANDOM + c * N_INTEGER:N_RANDOM + (c + 1) * N_INTEGER] = np.array(INT_TARGETS) + shift
    y[EQUAL0:TUBE0] = EQUAL_TARGET
    y[TUBE0:BOUND0] = TUBE_CENTRE + rng.uniform(-TUBE_HALF, TUBE_HALF, N_TUBE)
    y[BOUND0:] = np.where(np.arange(N_BOUND) % 2 == 0, 5.0, -5.0) + rng.uniform(-0.5, 0.5, N_BOUND)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def _own_stats(X, rows, shrink=1.0):
    mean, scale = X[rows].mean(axis=0), X[rows].std(axis=0) * shrink
    return mean, np.where(scale > 0, scale, 1.0)


def random_task(n_dims, n, C, seed, gamma, epsilon):
    """The task of a TRAJECTORY_SPECS entry: n of the 160 Gaussian samples, standardised with their own statistics."""
    X, _ = trajectory_matrix(n_dims)
    rows = np.random.default_rng(seed * 1000 + n).permutation(N_RANDOM)[:n]
    mean, scale = _own_stats(X, rows)
    return (rows, mean, scale, C, gamma, epsilon)


def integer_task(n_dims, samples, C, epsilon):
    """The task of a TAU_SPECS entry: integer samples 160 + s under mean 0 / scale 1."""
    return (N_RANDOM + np.array(samples), np.zeros(n_dims), np.ones(n_dims), C, None, epsilon)


@functools.lru_cache(maxsize=None)
def trajectory_tasks():
    """[Trajectory]: the random tasks of TRAJECTORY_SPECS, among them pairs that differ in epsilon alone and pairs that differ in
    gamma alone, and the TAU tasks of TAU_SPECS: integer rows, among them two rows that are the SAME point with different
    targets (samples 160 + k, 168 + k, 176 + k; a target belongs to a sample index, so the point is stored three times)."""
    out = []
    for n_dims, kernel, n, C, eps, seed, gamma, epsilon in TRAJECTORY_SPECS:
        name = "d%d_%s_n%d_C%g_s%d_e%g%s" % (n_dims, kernel, n, C, seed, epsilon, "" if gamma is None else "_g%g" % gamma)
        out.append(Trajectory(name, n_dims, kernel, eps, random_task(n_dims, n, C, seed, gamma, epsilon), False))
    for n_dims, name, samples, C, epsilon in TAU_SPECS:
        out.append(Trajectory("d%d_%s" % (n_dims, name), n_dims, "linear", 1e-3, integer_task(n_dims, samples, C, epsilon), True))
    return out


def trajectory_batches():
    """{(n_dims, kernel, eps): [Trajectory]}: what one svr_solve call can take together (it takes one eps)."""
    out = collections.OrderedDict()
    for t in trajectory_tasks():
        out.setdefault((t.n_dims, t.kernel, t.eps), []).append(t)
    return out


def standardised(X, task):
    """The rows of a task as the kernels read them."""
    return (X[task[0]] - task[1]) / task[2]


def same_point_rows(X, task):
    """[n] bool: the rows of a task that are the same point as another of its rows."""
    Z = X[task[0]]
    return np.array([np.count_nonzero(np.all(Z == z, axis=1)) > 1 for z in Z])


# ---------------------------------------------------------------------------------------------------------------------
# (b) exact ties at iteration 0
# ---------------------------------------------------------------------------------------------------------------------
TIE_C, TIE_TARGET = 4.0, 3.0
TIE_EPSILONS = (0.0, 0.5)               # exact in binary: every quantity of step 1 is exact but for the one division

TieLayout = collections.namedtuple("TieLayout", "name task i j n_top n_tied_j")


def tie_matrix():
    """(X, y): smo_edge_cases.tie_matrix() -- integer samples in 3 dims: 0 the origin, 1 the nearest other point (1, 1, 1),
    eta = 3; 2 .. 41 further points (-(k + 1), 1, 0); 42 .. 81 farther points (2 + k, 1, 1), eta >= 6 -- with the target +3
    where the SMO layouts have a positive row (samples 0 and 2 .. 41) and -3 where they have a negative one."""
    X = smo_edge_cases.tie_matrix()
    y = np.full(X.shape[0], TIE_TARGET)
    y[1] = -TIE_TARGET
    y[42:] = -TIE_TARGET
    return X, y


@functools.lru_cache(maxsize=None)
def tie_layouts():
    """[TieLayout]: the layouts of smo_edge_cases.tie_layouts() (row counts TIE_ROWS, positions from EDGE_POSITIONS, the kinds
    "one" and "scattered"), a positive row read as a row of the greatest target and a negative one as a row of the least.  At
    alpha = 0 only the variables t < n are in I_up, with v = y_t - epsilon: every row of the greatest target ties for i, and the
    greatest index p is to be chosen.  Only the variables t + n are in I_low, with b = y_max - y_t - 2 epsilon: the rows of the
    least target share b, the nearest sample among them has the least eta, and j is n + the greatest position holding it.
    Epsilon alternates between 0 and 0.5; C = 4 leaves the step 2 - 2 epsilon / 3 unclipped."""
    zeros, ones = np.zeros(smo_edge_cases.TIE_DIMS), np.ones(smo_edge_cases.TIE_DIMS)
    out = []
    for at, lay in enumerate(smo_edge_cases.tie_layouts()):
        rows = lay.task[0]
        epsilon = TIE_EPSILONS[at % 2]
        out.append(TieLayout("%s_e%g" % (lay.name, epsilon), (rows, zeros, ones, TIE_C, None, epsilon), lay.i, len(rows) + lay.j,
                             lay.n_positive, lay.n_tied_j))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# (c) degenerate tasks
# ---------------------------------------------------------------------------------------------------------------------
BOUND_C = 0.001


def degenerate_tasks(n_dims):
    """[(name, task)] over trajectory_matrix(n_dims).  Nothing to optimise (0 iterations, beta = 0): one row under epsilon 0
    and 0.1; eight rows of one target under epsilon 0 (a gap of exactly 0) and 0.1; twenty rows whose targets lie within the
    tube.  all_at_C: 40 targets near +5 and -5, rows scaled to |z|^2 of about 1, C = 0.001: 40 kernel values times 0.001
    cannot bring a prediction within epsilon of its target, so every beta ends at +-C."""
    X, _ = trajectory_matrix(n_dims)
    zeros, ones = np.zeros(n_dims), np.ones(n_dims)
    equal, tube, bound = np.arange(EQUAL0, TUBE0), np.arange(TUBE0, BOUND0), np.arange(BOUND0, N_SAMPLES)
    return [("one_e0", (np.array([5]), zeros, ones, 1.0, 0.3, 0.0)),
            ("one_e0.1", (np.array([77]), zeros, ones, 1.0, 0.3, 0.1)),
            ("equal_e0", (equal,) + _own_stats(X, equal) + (1.0, 0.3, 0.0)),
            ("equal_e0.1", (equal[::-1],) + _own_stats(X, equal) + (20.0, 0.3, 0.1)),
            ("in_tube", (tube,) + _own_stats(X, tube) + (1.0, 0.3, 0.1)),
            ("all_at_C", (bound,) + _own_stats(X, bound, np.sqrt(n_dims)) + (BOUND_C, 0.3, 0.1))]


ZERO_ITERATION = ("one_e0", "one_e0.1", "equal_e0", "equal_e0.1", "in_tube")


# ---------------------------------------------------------------------------------------------------------------------
# (d) sweep jobs
# ---------------------------------------------------------------------------------------------------------------------
SWEEP_DIMS, SWEEP_EPSILON = 9, 0.1
SweepCall = collections.namedtuple("SweepCall", "X y jobs names")


@functools.lru_cache(maxsize=None)
def sweep_call():
    """One svr_split_fit_predict call (RBF, gamma=None: every job its own 'scale' gamma) over trajectory_matrix(9):
    constant: the training rows are one point -- integer sample 3 and its twin, two targets -- under mean = the point: the
    standardised rows are all zero, their variance is 0 and gamma is exactly 1.0;
    C0.05, C1, C20: one training list, one test list, three values of C;
    own33, own12, own70: training lists under the statistics of all 160 Gaussian samples, as evaluate_regression scales: the
    variance of each list's standardised rows, hence its gamma, is its own."""
    X, y = trajectory_matrix(SWEEP_DIMS)
    rng = np.random.default_rng(41)
    jobs, names = [], []
    point = np.array([N_RANDOM + 3, N_RANDOM + N_INTEGER + 3] * 3)
    jobs.append((point, rng.permutation(N_RANDOM)[:5], X[point[0]].copy(), np.ones(SWEEP_DIMS), 1.0))
    names.append("constant")
    train, test = rng.permutation(N_RANDOM)[:40], rng.permutation(N_RANDOM)[:33]
    for C in (0.05, 1.0, 20.0):
        jobs.append((train, test) + _own_stats(X, train) + (C,))
        names.append("C%g" % C)
    for n, n_test in ((33, 31), (12, 1), (70, 32)):
        train = rng.permutation(N_RANDOM)[:n]
        jobs.append((train, rng.permutation(N_RANDOM)[:n_test]) + _own_stats(X, np.arange(N_RANDOM)) + (1.0,))
        names.append("own%d" % n)
    return SweepCall(X, y, jobs, names)


# ---------------------------------------------------------------------------------------------------------------------
# (e) max_iter against the launch budget
# ---------------------------------------------------------------------------------------------------------------------
BUDGET_DIMS, BUDGET_EPS = 9, 1e-1


def budget_tasks():
    """(a task of 45 iterations -- the trajectory task d9_linear_n47_C0.05_s31_e0 --, a two-row task that stops after one), both
    linear at eps = 0.1 over trajectory_matrix(9)."""
    return random_task(BUDGET_DIMS, 47, 0.05, 31, None, 0.0), random_task(BUDGET_DIMS, 2, 1.0, 0, None, 0.1)
