"""The shared cv::Mat float rules off the GPU: hand-made known answers for tests/cvmat_model.py (the Jacobi at every size the callers
use, the 3 x 3 inverse and the product), and orbslam2_amd/host/CvMat.h, driven by tests/cvmat_mirror/mirror_main.cpp, equal to the model
bit for bit -- built plain and as a stand-alone AddressSanitizer + UBSan program."""
import struct

import numpy as np
import pytest

from tests import cvmat_model as M
from tests import host_forms as H

F32, F64 = np.float32, np.float64
SIZES = [(3, 3), (4, 4), (9, 9), (9, 16)]      # (columns n, rows m): the rank-2 step and DecomposeE, Triangulate, ComputeF21, ComputeH21


# ------------------------------------------------------------------ known answers: the null vector
def _null(A):
    v, info = M.null_vector(np.array(A, F32))
    return [float(x) for x in v], info


def _e(k, n):
    return [1.0 if i == k else 0.0 for i in range(n)]


def _rows(square, m, offset=0):
    """An n x n matrix as m rows: zero rows around it."""
    A = np.zeros((m, square.shape[1]))
    A[offset:offset + len(square)] = square
    return A


def diagonal_matrices(n, m):
    """(matrix, column of the null vector, swaps of the selection sort)."""
    c = min(2, n - 2)
    out_of_place = np.arange(n, 0, -1.0)
    out_of_place[c] = 0.5                                           # orthogonal columns; the smallest is column c, every later one moves up
    ready = np.arange(n, 0, -1.0)
    ready[n - 1] = 0                                                # sorted already: Vt row n - 1 is the last unit vector
    cases = [(_rows(np.diag(out_of_place), m), c, n - 1 - c), (_rows(np.diag(ready), m), n - 1, 0),
             (_rows(np.diag(np.arange(n) * 1.0), m), 0, n // 2),    # ascending: the selection sort swaps (0, n - 1), (1, n - 2), ...
             (_rows(np.eye(n), m), n - 1, 0)]                       # equal singular values: strict < keeps the first, the LAST of the equals ends in row n - 1
    if m > n:                                                       # the block in the middle of the rows, as in ComputeH21's 16 x 9 matrix
        d = np.arange(n, 0, -1.0)
        d[4] = 0.25
        cases.append((_rows(np.diag(d), m, (m - n) // 2), 4, n - 1 - 4))
    return cases


def two_column_matrices(n, m):
    """A: columns 0 and 1 equal, the kernel is (1, -1, 0, ...) / sqrt(2).  B: |col 0|^2 = 1 < |col 1|^2 = 5.  Bs: B with the two swapped."""
    A = np.diag([0.0, 0.0] + list(range(3, n + 1)))
    A[0, :2] = 1
    A[1, :2] = 2
    B = np.diag([1.0, 1.0] + list(range(3, n + 1)))
    B[0, 1] = 2
    return _rows(A, m), _rows(B, m), _rows(B[:, [1, 0] + list(range(2, n))], m)


def random_matrix(n, m):
    rng = np.random.default_rng(3)
    tall, square = rng.normal(size=(16, n)).astype(F32), rng.normal(size=(n, n)).astype(F32)
    return tall if m == 16 else square


def short_matrices(n, m):
    """n - 1 random rows, and the same padded with zero rows to n, m and 16 rows."""
    A = np.random.default_rng(4).normal(size=(n - 1, n)).astype(F32)
    return [A] + [np.concatenate([A, np.zeros((rows - n + 1, n), F32)]) for rows in (n, m, 16)]


@pytest.mark.parametrize("n,m", SIZES)
def test_null_vector_of_a_diagonal_matrix_needs_no_rotation_and_only_the_sort(n, m):
    for A, column, swaps in diagonal_matrices(n, m):
        v, info = _null(A)
        assert v == _e(column, n) and info["rotations"] == 0 and info["sweeps"] == 0 and info["swaps"] == swaps, (A, v, info)
        assert info["first_beta_negative"] is None


@pytest.mark.parametrize("n,m", SIZES)
def test_null_vector_first_rotation_takes_either_branch_of_beta(n, m):
    A, B, Bs = two_column_matrices(n, m)
    v, info = _null(A)
    assert info["first_beta_negative"] is False and info["rotations"] >= 1        # equal norms: beta == 0 takes the else branch
    assert abs(abs(v[0]) - 2 ** -0.5) < 1e-6 and abs(v[0] + v[1]) < 1e-6 and v[2:] == [0.0] * (n - 2)
    assert _null(B)[1]["first_beta_negative"] is True
    assert _null(Bs)[1]["first_beta_negative"] is False
    # full rank: Vt row n - 1 is the right singular vector of the smallest singular value
    for mat, tol in ((B, 1e-6), (Bs, 1e-6), (random_matrix(n, m), 2e-6)):
        v = np.array(_null(mat)[0])
        want = np.linalg.svd(np.asarray(mat, np.float64))[2][n - 1]
        assert min(np.abs(v - want).max(), np.abs(v + want).max()) < tol


@pytest.mark.parametrize("n,m", SIZES)
def test_a_matrix_one_row_short_is_padded_with_a_zero_row(n, m):
    """ComputeF21's 8 x 9 matrix: the contract pads a zero row.  More zero rows change no bit (x + 0 * 0 == x), which is what lets the
    kernel run both models on one 16-entry row stride; the answer spans the null space of the n - 1 rows."""
    A = short_matrices(n, m)[0]
    (v, info), padded = M.null_vector(A), [M.null_vector(P)[0] for P in short_matrices(n, m)[1:]]
    assert all(np.array_equal(H.bits(v), H.bits(p)) for p in padded)
    assert abs(np.linalg.norm(v.astype(np.float64)) - 1) < 1e-6 and np.abs(A.astype(np.float64) @ v).max() < 2e-6
    # a column of exact rank deficiency never meets the relative test, so the sweep cap ends it -- unless a rotation leaves the column
    # exactly zero (|p| = 0 <= 0 then holds), which two rows can do (n = 3) and ComputeF21's eight do not
    with np.errstate(all="ignore"):
        W = M.jacobi(M.transposed(A, n), n, n)[2]
    assert info["sweeps"] == M.MAX_SWEEPS or (W[0, n - 1] == 0 and n == 3)


def test_the_batched_jacobi_equals_one_matrix_at_a_time():
    """Arrays run across independent problems only: a batch of 40 random 4 x 4 matrices gives the bits of 40 single calls."""
    A = np.random.default_rng(5).normal(size=(40, 4, 4)).astype(F32)
    At = np.concatenate([M.transposed(a, 4) for a in A])
    with np.errstate(all="ignore"):
        batch = M.jacobi(At, 4, 4)
        for b in range(40):
            one = M.jacobi(At[b:b + 1], 4, 4)
            assert all(np.array_equal(H.bits(batch[k][b]), H.bits(one[k][0])) for k in range(3))
            assert all(batch[3][k][b] == one[3][k][0] for k in batch[3])


# ------------------------------------------------------------------ known answers: 3 x 3 steps
SINGULAR = np.array([[1, 2, 3], [2, 4, 6], [0, 0, 0]], F32)
ZERO_COLUMN = np.array([[1, 0, 2], [3, 0, 4], [5, 0, 7]], F32)


def test_the_inverse_is_opencv_s_closed_form_and_a_zero_determinant_gives_the_zero_matrix():
    assert np.array_equal(M.inv3(np.diag([2.0, 4.0, 8.0]).astype(F32)), np.diag([0.5, 0.25, 0.125]).astype(F32))
    assert np.array_equal(M.inv3(SINGULAR), np.zeros((3, 3), F32))
    one_row = np.zeros((3, 3), F32); one_row[0] = [203.65, 0.1, 0.84]
    assert np.array_equal(M.inv3(one_row), np.zeros((3, 3), F32))
    mx, my, sx, sy = F32(310.5), F32(236.25), F32(0.0078125), F32(0.0107421875)
    T = np.array([[sx, 0, -mx * sx], [0, sy, -my * sy], [0, 0, 1]], F32)          # Normalize's T: the inverse is (1 / sX, 1 / sY, meanX, meanY)
    want = np.array([[128.0, 0, 310.5], [0, 1 / 0.0107421875, 236.25], [0, 0, 1]])
    assert np.allclose(M.inv3(T), want, rtol=1e-7)
    batch = np.stack([SINGULAR, np.diag([2.0, 4.0, 8.0]).astype(F32)])
    assert np.array_equal(M.inv3(batch)[0], np.zeros((3, 3), F32)) and M.inv3(batch)[1][0, 0] == 0.5
    a, b = np.arange(9, dtype=F32).reshape(3, 3), np.array([[1, 0, 2], [0, 3, 0], [4, 0, 5]], F32)
    assert np.array_equal(M.mat(a, b), (a.astype(np.float64) @ b.astype(np.float64)).astype(F32))


# ------------------------------------------------------------------ the C++ host form
def jacobi_inputs():
    """Every matrix of the known answers above with at least as many rows as columns, at the four sizes, and the zero column."""
    mats = []
    for n, m in SIZES:
        mats += [A for A, _, _ in diagonal_matrices(n, m)] + list(two_column_matrices(n, m)) + [random_matrix(n, m)] + short_matrices(n, m)[1:]
    return [np.asarray(A, F32) for A in mats] + [ZERO_COLUMN]


def small_inputs():
    """(a, b, plus, alpha) for the 3 x 3 steps: general matrices, the zero column (W = 0: the FLT_MIN branch of Svd3) and the singular one."""
    rng = np.random.default_rng(6)
    a = [rng.normal(size=(3, 3)).astype(F32) for _ in range(3)] + [ZERO_COLUMN, SINGULAR, np.diag([2.0, 4.0, 8.0]).astype(F32)]
    return [(x, rng.normal(size=(3, 3)).astype(F32), rng.normal(size=(3, 3)).astype(F32), float(alpha)) for x, alpha in zip(a, (1.0, -1.0, 0.37, 2.5, -0.125, 3.0))]


STORED = np.array([0x3F800000, 0x7FC00000, 0xFFC12345, 0x7F800001, 0x7F800000, 0x80000000], np.uint32).view(F32)


SEEDED = 2048                                   # added matrices per size


def seeded_jacobi_inputs(n, m, count=SEEDED):
    """float32[count][m][n], seeded, for the three-way agreement of model, host form and device forms (tests/test_arith_blocks.py): a quarter
    with a duplicated column, an eighth with a zero column, an eighth one row short (n - 1 random rows, the rest zero), and in the general
    half one matrix with a NaN entry and one with an Inf entry."""
    rng = np.random.default_rng(1000 * n + m)
    A = rng.normal(size=(count, m, n)).astype(F32)
    q, e = count // 4, count // 8
    src, dst = rng.integers(0, n, q), rng.integers(1, n, q)
    dst = (src + dst) % n                                           # another column
    A[np.arange(q), :, dst] = A[np.arange(q), :, src]
    A[np.arange(q, q + e), :, rng.integers(0, n, e)] = 0
    A[q + e:q + 2 * e, n - 1:, :] = 0
    A[q + 2 * e, m // 2, n // 2] = np.nan
    A[q + 2 * e + 1, 0, n - 1] = np.inf
    return A


def seeded_small_inputs(count=4096):
    """(a, b, plus, alpha) arrays for the 3 x 3 steps: `count` seeded full-mantissa matrices, then 512 each of matrices whose determinant
    expression is exactly 0 (small integers with row 2 = row 0 + row 1: every product and sum is exact), matrices with two equal
    full-mantissa rows (each cofactor is x * y - y * x = 0) and nearly singular ones (the equal-row
    matrices with one entry moved by one ulp; and full-mantissa matrices with row 2 = fl(row 0 + row 1), whose determinant of about 1e-8
    is what cancellation leaves of terms of order 1, so that a last-bit change of one term moves the inverse), and the STORED patterns."""
    rng = np.random.default_rng(7)
    a = rng.normal(size=(count, 3, 3)).astype(F32)
    ints = rng.integers(-1000, 1001, size=(512, 3, 3)).astype(F32)
    ints[:, 2] = ints[:, 0] + ints[:, 1]
    twin = rng.normal(size=(512, 3, 3)).astype(F32)
    twin[:, 2] = twin[:, 1]
    near = rng.normal(size=(512, 3, 3)).astype(F32)
    near[:, 2] = near[:, 1]
    k = rng.integers(0, 3, 512)
    near[np.arange(512), 2, k] = np.nextafter(near[np.arange(512), 2, k], F32(np.inf))
    cancel = rng.normal(size=(512, 3, 3)).astype(F32)
    cancel[:, 2] = cancel[:, 0] + cancel[:, 1]
    pat = np.stack([np.roll(np.resize(STORED, 9), r).reshape(3, 3) for r in range(len(STORED))])
    a = np.concatenate([a, ints, twin, near, cancel, pat])
    b, plus = rng.normal(size=a.shape).astype(F32), rng.normal(size=a.shape).astype(F32)
    alpha = rng.normal(size=len(a))
    return a, b, plus, alpha


def write_problem_file(path):
    with open(path, "wb") as f:
        J, S3 = jacobi_inputs(), small_inputs()
        J = J + [A for n, m in SIZES for A in seeded_jacobi_inputs(n, m)]
        S3 = S3 + list(zip(*seeded_small_inputs()))
        f.write(struct.pack("<i", len(J)))
        for A in J:
            f.write(struct.pack("<ii", A.shape[1], A.shape[0]) + A.tobytes())
        f.write(struct.pack("<i", len(S3)))
        for a, b, plus, alpha in S3:
            f.write(a.tobytes() + b.tobytes() + plus.tobytes() + struct.pack("<d", alpha))
        f.write(struct.pack("<i", len(STORED)) + STORED.tobytes())


def _jacobi_expected(q0, As):
    """One batched call of the model for matrices of one shape (the batch gives the bits of single calls, as tested above)."""
    m, n = As[0].shape
    At, Vt, W, info = M.jacobi(np.concatenate([M.transposed(A, n) for A in As]), n, m)
    out = []
    for b in range(len(As)):
        out += [("jacobi %d (%d x %d) %s" % (q0 + b, m, n, k), v)
                for k, v in (("At", At[b]), ("Vt", Vt[b]), ("W", W[b]), ("sweeps", info["sweeps"][b:b + 1].astype(np.int32)))]
    return out


def _small_expected(q0, a, b, plus, alpha):
    u, w, vt, _ = M.svd3(a)
    inv, ab, abp, det, norm = M.inv3(a), M.mat(a, b), M.mat(a, b, alpha=float(alpha[0]) if len(a) == 1 else np.asarray(alpha, F64), plus=plus), M.det3(a), M.norm(a[:, 0])
    out = []
    for i in range(len(a)):
        steps = (("u", u[i]), ("w", w[i]), ("vt", vt[i]), ("inv", inv[i]), ("ab", ab[i]), ("abp", abp[i]), ("unit", M.unit(a[i, 0])),
                 ("det", det[i:i + 1]), ("norm", norm[i:i + 1]))
        out += [("3 x 3 %d %s" % (q0 + i, k), v) for k, v in steps]
    return out


@pytest.fixture(scope="module")
def expected():
    """What the model gives for the problem file, in the order of the result file: a list of (name, array)."""
    out = []
    with np.errstate(all="ignore"):
        for q, A in enumerate(jacobi_inputs()):
            out += _jacobi_expected(q, [A])
        q = len(jacobi_inputs())
        for n, m in SIZES:
            out += _jacobi_expected(q, list(seeded_jacobi_inputs(n, m)))
            q += SEEDED
        S3 = small_inputs()
        for q, (a, b, plus, alpha) in enumerate(S3):
            out += _small_expected(q, a[None], b[None], plus[None], [alpha])
        out += _small_expected(len(S3), *seeded_small_inputs())
        out.append(("stored", M.stored(STORED)))
    return out


def test_the_inputs_of_the_host_form_reach_the_branches_they_are_there_for(expected):
    got = dict(expected)
    assert got["3 x 3 3 w"][2] == 0 and not got["3 x 3 3 u"][:, 2].any() and got["3 x 3 3 u"][:, :2].any()      # W = 0: u's column is 0, not 1 / 0
    assert not got["3 x 3 3 inv"].any() and not got["3 x 3 4 inv"].any() and got["3 x 3 3 det"][0] == 0         # singular: the zero matrix
    assert got["3 x 3 0 inv"].all() and got["3 x 3 5 inv"][0, 0] == 0.5
    assert got["stored"].view(np.uint32).tolist() == [0x3F800000, M.NAN_BITS, M.NAN_BITS, M.NAN_BITS, 0x7F800000, 0x80000000]
    sweeps = [int(v[0]) for k, v in expected if k.endswith("sweeps")]
    assert 0 in sweeps and M.MAX_SWEEPS in sweeps and any(0 < s < M.MAX_SWEEPS for s in sweeps)


@pytest.mark.parametrize("build", H.BUILDS)
def test_cpp_host_form_equals_the_model_bit_for_bit(tmp_path, build, expected):
    exe = H.build(tmp_path, "cvmat_mirror", build)
    problem, result = str(tmp_path / "problem.bin"), str(tmp_path / "out.bin")
    write_problem_file(problem)
    H.run(exe, problem, result)
    raw = open(result, "rb").read()
    at = 0
    for name, want in expected:
        want = np.ascontiguousarray(want)
        got = raw[at:at + want.nbytes]
        at += want.nbytes
        if name != "stored" and want.dtype.kind == "f" and np.isnan(want).any():     # the payload of a computed NaN is the processor's
            got, want = H.bits_one_nan(np.frombuffer(got, want.dtype)).tobytes(), np.frombuffer(H.bits_one_nan(want).tobytes(), want.dtype)
        assert got == want.tobytes(), "%s differs: %s, model %s" % (name, np.frombuffer(got, want.dtype).tolist(), want.reshape(-1).tolist())
    assert at == len(raw)


def test_the_host_header_includes_nothing_of_the_project_but_the_c_abi_header():
    assert H.project_includes(H.header("CvMat.h")) in ([], H.ABI_AND_CVMAT[:1])
    text = open(H.header("CvMat.h")).read().lower()
    assert "opencv2" not in text and "hip/" not in text and "#include <opencv" not in text
