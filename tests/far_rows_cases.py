"""Cases of the far-row tests (tests/test_far_rows_host.py without a GPU, tests/test_gpu_far_rows.py on one): the row contract
of tests/row_contract_cases.py -- "rows as they lie" -- stretched to "rows wherever they lie": the same families and shapes,
with ONE matrix of a call placed so that its rows start on both sides of every point at which a 32-bit offset wraps.

Thresholds, as the float index of a row's first element counted from the matrix's base pointer (what a kernel multiplies:
``row * stride``):

    B1 = 2^29   a signed 32-bit BYTE offset wraps
    B2 = 2^30   an unsigned 32-bit byte offset wraps: the range of a buffer descriptor
    B3 = 2^31   a signed 32-bit ELEMENT index wraps
    B4 = 2^32   an unsigned 32-bit element index wraps

A far placement of a matrix of ``rows`` rows is ``(stride, offset)``, a function of ``rows`` alone: row k starts k * stride
floats behind the base, the base ``offset`` floats into the buffer.  Row 0 starts below B1, the last row at or above B4, and
with stride < 2^29 at least one row starts inside each of [B1, B2), [B2, B3) and [B3, B4).  An offset that lost its upper
bits -- the whole product, or one term of it (t * S * stride wrapped, s * stride added) -- lands m * 2^30 floats below the true
row for some m >= 1.  So the strides are chosen such that the rows' starts, taken modulo 2^30, lie at least MAX_COLS apart on
the circle: a wrapped access of at most MAX_COLS floats then never meets a row of the same matrix, another one or its own;
it meets the filling between the rows (a sentinel, or NaN under a matrix that is read) or leaves the buffer in front.
Two placements per matrix: ``vector`` (stride a multiple of 8, offset 0: the 16-byte path for float32 and for 16-bit
elements) and ``scalar`` (an odd stride, the base one element off: the four-dword path).  Importing this module needs no GPU."""
import functools
from collections import namedtuple

import numpy as np
import torch

from torchain_amd import synth

import row_contract_cases as rc

B1, B2, B3, B4 = 1 << 29, 1 << 30, 1 << 31, 1 << 32
THRESHOLDS = (B1, B2, B3, B4)
MAX_COLS = 1 << 15   # no matrix of these tests is wider (the widest: 9000 pdfs; a joint head of two halves: 2 * 100)
SLACK = rc.SLACK
PATHS = ("vector", "scalar")

Placement = namedtuple("Placement", "path stride offset")


def row_starts(rows, stride):
    return [k * stride for k in range(rows)]


def covers(rows, stride):
    """The coverage conditions on the rows' first elements (indices from the base pointer)."""
    starts = row_starts(rows, stride)
    return (starts[0] < B1 and starts[-1] >= B4
            and all(any(lo <= s < hi for s in starts) for lo, hi in ((B1, B2), (B2, B3), (B3, B4))))


def wrapped_clear(rows, stride, width=MAX_COLS):
    """No two rows' starts are closer than ``width`` modulo 2^30 (2^31 and 2^32 are multiples of it): row k's offset less any
    m * 2^30, m >= 1, is then at least ``width`` away from every row's start, its own included."""
    res = sorted(s % B2 for s in row_starts(rows, stride))
    gaps = [b - a for a, b in zip(res, res[1:])] + [res[0] + B2 - res[-1]]
    return min(gaps) >= width


@functools.lru_cache(maxsize=None)
def far_placement(rows, path):
    """The smallest stride at or above B4 / (rows - 1) of the path's kind that meets both conditions."""
    assert rows >= 10 and path in PATHS, (rows, path)   # (fewer rows: a stride below 2^29 does not reach B4)
    stride = -(-B4 // (rows - 1))
    if path == "vector":
        stride, step, offset = (stride + 7) & ~7, 8, 0
    else:
        stride, step, offset = stride | 1, 2, 1
    while not (covers(rows, stride) and wrapped_clear(rows, stride)):
        stride += step
    assert stride < B1
    return Placement(path, stride, offset)


def buffer_numel(rows, cols, placement):
    """Elements of the buffer that holds the matrix: up to the last row's last element, and SLACK behind it."""
    assert cols <= MAX_COLS
    return placement.offset + (rows - 1) * placement.stride + cols + SLACK


def far(rows, cols, placement, fill, device, dtype=torch.float32, pool=None):
    """(buffer, view): a flat tensor of ``buffer_numel`` elements filled with ``fill`` and the (rows, cols) matrix in it.
    ``pool``: a flat tensor of at least that many elements to take the buffer from (its first elements), so that a test
    which places several matrices far in turn allocates once."""
    numel = buffer_numel(rows, cols, placement)
    if pool is None:
        buffer = torch.full((numel,), float(fill), dtype=dtype, device=device)
    else:
        assert pool.dim() == 1 and pool.dtype == dtype and pool.numel() >= numel
        buffer = pool[:numel].fill_(float(fill))
    return buffer, buffer.as_strided((rows, cols), (placement.stride, 1), placement.offset)


def pool_numel(rows, cols):
    """Elements of a pool that serves both placements of the matrix."""
    return max(buffer_numel(rows, cols, far_placement(rows, path)) for path in PATHS)


# One size for every test's pool, in float32 elements (17.2 GB; a 16-bit matrix takes half of it): (rows - 1) * stride passes
# 2^32 by less than rows * 8.  Blocks of one size are what an allocator that caches can hand out again.
POOL_NUMEL = B4 + (1 << 20)


def near(rows, cols, path, fill, device, dtype=torch.float32):
    """The same for a matrix that stays near: the row contract's padded rows on the same path."""
    pad, offset = (8, 0) if path == "vector" else (3, 1)
    buffer = torch.full((offset + rows * (cols + pad) + SLACK,), float(fill), dtype=dtype, device=device)
    return buffer, buffer.as_strided((rows, cols), (cols + pad, 1), offset)


def on_path(view, path):
    """Whether the view lies as the path asks (api.cpp's rule for float32, layout_kernels.hip's for 16-bit elements)."""
    lane = 16 // view.element_size()
    vec = view.shape[1] % lane == 0 and view.stride(0) % lane == 0 and view.data_ptr() % 16 == 0
    return vec == (path == "vector")


def need_bytes(rows, cols, placement, element_size=4):
    return buffer_numel(rows, cols, placement) * element_size


# ---- the history at size -----------------------------------------------------------------------------------------------
# One case per kernel family that keeps a history of alpha: the smallest (S, T) at which (T + 1) * S * Hs floats pass 2^31.
# Hs: stored states per frame and sequence -- 4096 for the 300-state graph on the fused tied and on the owner-computes
# general kernel (whole planes), 20480 for the smallest plane-wise graph, the states themselves on the streamed path, whose
# batch is padded to whole slabs of 32 sequences (Sp).  Where the family's own graph would cost the CPU oracle many seconds
# (its cost is arcs x frames x sequences, and 2^31 state-frames are the least it can have) the graph is ``thin_den_fst``: one
# self-loop and one forward arc per state.  Two things it keeps from the graphs whose at-size runs the suite's element-wise
# bound (1e-4 relative on entries above 1e-3: 1e-7 absolute) was set on, C3 and X2 with 8 and 10 arcs per state:
#   * the self-loop's share of a state's probability, 1/8.  The tied kernels form a state's forward occupation as a
#     difference, beta * (alpha_{t+1} - self-loop part); its relative rounding error is eps * alpha / (alpha - self-loop
#     part), which grows with that share (random_den_fst with two arcs would give the self-loop 1/2 on average);
#   * few adds per element of gamma_t: a state's occupations are added in unsigned fixed point with 31 fractional bits, up
#     to 2^-31 of rounding per add, so the bound leaves room for about 200.  2 * states / pdfs is 55 and 60 here (the
#     family graph "planes": 57); with 64 pdfs it would be 512.
def thin_den_fst(num_states, num_pdfs, seed):
    fst = synth.random_den_fst(num_states, 2, num_pdfs, seed=seed)
    prob = np.tile(np.array([0.125, 0.875]), num_states)        # arcs are state-major: the self-loop, then the forward arc
    assert np.array_equal(fst.src[0::2], fst.dst[0::2])
    return fst._replace(weight=(-np.log(prob)).astype(np.float32))


AtSize = namedtuple("AtSize", "name graph build launch tied S T Hs Sp")
AT_SIZE_GRAPHS = {
    "tied8": rc.GRAPHS["tied8"],
    "planes_thin": (thin_den_fst, (16400, 600), dict(seed=81)),
    "streamed_thin": (thin_den_fst, (30000, 1000), dict(seed=82)),
}
AT_SIZE = (
    AtSize("fused_tied", "tied8", (), ("no_phase_split",), 1, 2048, 256, 4096, 2048),
    AtSize("plane_wise", "planes_thin", (), ("no_phase_split",), 1, 512, 205, 20480, 512),
    AtSize("general_owner", "tied8", ("force_general",), (), 0, 2048, 256, 4096, 2048),
    AtSize("streamed", "streamed_thin", ("force_streamed", "slab_wide"), (), 2, 257, 250, 30000, 288),
)


@functools.lru_cache(maxsize=None)
def at_size_fst(graph):
    make, args, kwargs = AT_SIZE_GRAPHS[graph]
    return make(*args, **kwargs)


def history_floats(case):
    return (case.T + 1) * case.Sp * case.Hs


# ---- the step ----------------------------------------------------------------------------------------------------------
# 24 pdfs (whole 16-byte lanes of float32 and of 16-bit elements), 3 sequences of 5 frames: 15 rows, odd B and T.  Input and
# xent_input share their strides, so both live in ONE far buffer, a joint head: row r holds the chain output in its first P
# elements and the xent output in the next P.
STEP_P, STEP_B, STEP_T = 24, 3, 5


def channel_last_strides(major, B, T, stride):
    """(batch_stride, frame_stride) of a channel-last view whose B * T rows lie ``stride`` apart: ``batch`` -- (B, T, C), row
    b * T + t -- or ``time`` -- (T, B, C), row t * B + b."""
    return (T * stride, stride) if major == "batch" else (stride, B * stride)


def strides_ok(B, T, cols, sb, st):
    """layout_rows_kernels.hip's channel_last_strides_ok restated in Python integers."""
    if B <= 0 or T <= 0 or cols <= 0 or (B > 1 and sb < cols) or (T > 1 and st < cols):
        return False
    if B == 1 or T == 1:
        return True
    lim = (2 ** 63 - 1) // 4
    if sb > lim // T or st > lim // B:
        return False
    return sb >= (T - 1) * st + cols or st >= (B - 1) * sb + cols


def adds_per_entry(fst):
    """Fixed-point adds into one element of gamma_t, on average: every state adds its self-loop's and its entering arcs'
    occupation (tied kernels), or every arc its own (general kernels)."""
    return max(2 * fst.num_states, len(fst.src)) / fst.num_pdfs


# How much worse than the median eighth of the frames the first or the last eighth of an at-size case may be, in worst absolute
# error and in worst relative error above 1e-3.  It rests on two allowances, not on a measurement.  Depth: rounding accumulates
# at most linearly along a recursion, and an end lies up to T frames from where one of the two recursions starts, the middle
# T / 2 from both: a factor 2.  Extremes: each figure is the maximum over one eighth of the entries, and the relative one is
# carried by the few entries just above 1e-3, where one absolute rounding weighs most; maxima of equally large samples of
# such a quantity differ by small multiples, allowed for with a factor 4.  2 * 4 = 8.  What the check is for is far beyond
# it: rows of alpha read from another frame's place give posteriors wrong by their own size, 1e-2 to 1, against a median
# near 1e-6 -- four orders of magnitude.
ENDS_FACTOR = 8.0

# The other matrices the GPU module places far, as (what, rows, cols) or what gives them, for the host module's proof
XENT_SHAPE = (85, 100)                # tc_xent_objf's two matrices
NUM_REGULAR = "single_path_150"       # of num_elementwise_cases.SINGLE_PATH: resident, and windowed under force_num_windowed
NUM_E2E = "random_7x37"               # of num_elementwise_cases.E2E
