"""Cases of the row-contract tests (tests/test_gpu_row_contract.py on the GPU, tests/test_row_contract_host.py without one):
what every denominator kernel form does with the caller's (rows, cols, row_stride) matrices as they are handed over --
non-finite values ("NaN / inf inputs still fail softly"; include/torchain_hip.h: "on NaN/inf ... objf =
-10*weight") and rows that are not ``cols`` apart or not 16-byte aligned (api.cpp: y_vec, d_vec, x_vec).

One ``Family`` per kernel form: a seeded graph from ``synth``, the ``tc_debug_set`` switches that put it on that form (those
read when a graph is BUILT and those read at LAUNCH, include/torchain_hip.h), the ``stats()["tied"]`` it must report
(0 general, 1 tied on chip, 2 streamed) and the batch.  Shapes are the smallest that reach each instantiation: 3 sequences of
7 frames on chip (an odd batch, a phantom partner for the two-sequence kernel, meeting frame 3), 17 x 5 / 33 x 5 for slabs of
16 / 32 sequences (one sequence past a whole slab).  Importing this module needs no GPU."""
import functools
from collections import namedtuple

import numpy as np
import torch

from torchain_amd import io, synth

LEAKY = 0.1

Family = namedtuple("Family", "name graph build launch tied S T")

# name -> (generator, arguments); seeded, built once per process (``den_fst``)
GRAPHS = {
    "tied8": (synth.random_den_fst, (300, 4, 100), dict(seed=4)),            # <= 8192 positions: 8 states per thread
    "tied12": (synth.random_den_fst, (9000, 6, 1500), dict(seed=23)),        # 12 states per thread
    "tied16": (synth.random_den_fst, (13000, 5, 2928), dict(seed=24)),       # 16 states per thread
    "pdfs2": (synth.random_den_fst, (300, 4, 4100), dict(seed=25)),          # two planes of pdfs, a partial last vector
    "pdfs3": (synth.random_den_fst, (300, 4, 9000), dict(seed=26)),          # three planes of pdfs
    "planes": (synth.random_den_fst, (17000, 3, 600), dict(seed=77)),        # plane-wise kernel
    "split": (synth.random_den_fst, (30000, 3, 600), dict(seed=78)),         # gather source in LDS a half at a time
    "skewed": (synth.skewed_den_fst, (80, 900, 40), dict(seed=5)),           # a general graph, naturally
    # P % 4 != 0 (bad values only: there is no vector path): a ragged last float4
    "ragged4097": (synth.random_den_fst, (300, 4, 4097), dict(seed=27)),
    "ragged77": (synth.random_den_fst, (300, 4, 77), dict(seed=28)),
    # 2 * 40 arcs' labels over 200 pdfs: most columns are carried by no arc
    "unused": (synth.random_den_fst, (40, 3, 200), dict(seed=29)),
}

ON_CHIP = (3, 7)
NARROW = (17, 5)
WIDE = (33, 5)


def _f(name, graph, build=(), launch=(), tied=1, batch=ON_CHIP):
    return Family(name, graph, tuple(build), tuple(launch), tied, batch[0], batch[1])


# every denominator kernel form, all with P % 4 == 0 (so that a 16-byte row path exists)
FAMILIES = (
    _f("tied8_two_cu", "tied8"),
    _f("tied8_mitm", "tied8", launch=("force_mitm",)),
    _f("tied8_no_mitm", "tied8", launch=("no_mitm",)),
    _f("tied8_fused", "tied8", launch=("no_phase_split",)),
    _f("tied8_pair", "tied8", launch=("force_pair",)),
    _f("tied12_two_cu", "tied12"),
    _f("tied12_fused", "tied12", launch=("no_phase_split",)),
    _f("tied16_two_cu", "tied16"),
    _f("tied16_fused", "tied16", launch=("no_phase_split",)),
    _f("pdfs2_fused", "pdfs2", launch=("no_phase_split",)),
    _f("pdfs3_fused", "pdfs3", launch=("no_phase_split",)),
    _f("planes_two_cu", "planes"),
    _f("planes_fused", "planes", launch=("no_phase_split",)),
    _f("split_two_cu", "split"),
    _f("split_fused", "split", launch=("no_phase_split",)),
    _f("streamed_narrow", "tied8", build=("force_streamed", "slab_narrow"), tied=2, batch=NARROW),
    _f("streamed_wide", "tied8", build=("force_streamed", "slab_wide"), tied=2, batch=WIDE),
    _f("general_owner", "tied8", build=("force_general",), tied=0),
    _f("general_old", "tied8", build=("force_general", "old_general"), tied=0),
    _f("general_natural", "skewed", tied=0),
)

# further forms and graphs for the bad values alone: exp(y) transposed a frame at a time, the general streamed kernels, ragged
# last vectors, a graph with unused pdfs on every mechanism (two-CU and fused tied, streamed, both general kernels)
BAD_VALUE_ONLY = (
    _f("streamed_narrow_per_frame", "tied8", build=("force_streamed", "slab_narrow"), launch=("exp_per_frame",), tied=2, batch=NARROW),
    _f("streamed_general", "skewed", build=("force_streamed", "slab_narrow"), tied=2, batch=NARROW),
    _f("ragged4097_fused", "ragged4097", launch=("no_phase_split",)),
    _f("ragged77_two_cu", "ragged77"),
    _f("ragged77_streamed", "ragged77", build=("force_streamed", "slab_narrow"), tied=2, batch=NARROW),
    _f("ragged77_general_old", "ragged77", build=("force_general", "old_general"), tied=0),
    _f("unused_two_cu", "unused"),
    _f("unused_fused", "unused", launch=("no_phase_split",)),
    _f("unused_streamed", "unused", build=("force_streamed", "slab_wide"), tied=2, batch=WIDE),
    _f("unused_general_owner", "unused", build=("force_general",), tied=0),
    _f("unused_general_old", "unused", build=("force_general", "old_general"), tied=0),
)

BAD_VALUE_FAMILIES = FAMILIES + BAD_VALUE_ONLY
# the whole objective on strided matrices: the fused tied and the plane-wise form write xent_deriv's zero rows themselves
# (x_vec), the streamed and the general form have it cleared in front
OBJECTIVE_FAMILIES = tuple(f for f in FAMILIES if f.name in ("tied8_fused", "planes_fused", "streamed_narrow", "general_owner"))
assert len(OBJECTIVE_FAMILIES) == 4

BY_NAME = {f.name: f for f in BAD_VALUE_FAMILIES}
assert len(BY_NAME) == len(BAD_VALUE_FAMILIES)


@functools.lru_cache(maxsize=None)
def den_fst(graph):
    make, args, kwargs = GRAPHS[graph]
    return make(*args, **kwargs)


_graphs = {}


def den_graph(family, force):
    """The family's ``io.DenominatorGraph``, built once per process and set of build-time switches.  ``force``: the
    ``kernel_family`` fixture; the family's build-time and launch-time switches and ``no_tune`` are set for the calling test
    whether the graph is new or not."""
    force("no_tune")
    for key in family.build + family.launch:
        force(key)
    key = (family.graph, family.build)
    if key not in _graphs:
        fst = den_fst(family.graph)
        _graphs[key] = io.DenominatorGraph(fst, fst.num_pdfs)
    return _graphs[key]


@functools.lru_cache(maxsize=None)
def nnet_output(graph, S, T):
    """Seeded outputs of the case, (T * S, P) float32, read-only: shared by the tests."""
    y = synth.random_nnet_output(S, T, den_fst(graph).num_pdfs, seed=1000 + S)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def initial_probs(graph):
    """The CPU oracle's 100-iteration estimate (not the library's own), as ``helpers.peaky_check`` takes it."""
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle.DenGraph(den_fst(graph)).initial_probs()


@functools.lru_cache(maxsize=None)
def float64_reference(graph, S, T):
    """(log-prob, occupation matrix) of the case in float64, oracle/independent_f64.py on clip(y, -30, 30) as in
    ``helpers.peaky_check``; computed once and read-only."""
    from oracle import independent_f64 as ind
    fst = den_fst(graph)
    pi = initial_probs(graph)
    lp, gam = ind.den_logprob_and_deriv(fst, pi, np.clip(nnet_output(graph, S, T), -30.0, 30.0), S, LEAKY)
    gam = np.asarray(gam, np.float64)
    gam.setflags(write=False)
    return lp, gam


@functools.lru_cache(maxsize=None)
def supervision(graph, S, T, weight=0.5):
    return synth.random_supervision(den_fst(graph), S, T, 2, seed=77 + S, weight=weight, initial_probs=initial_probs(graph))


def carried(sup):
    """Boolean (T * S, P): the entries some numerator arc carries.  The merged supervision is time-sorted: a state of time
    tau emits frame tau % T of sequence tau // T, row (tau % T) * S + tau // T (oracle/independent_f64.py: num_logprob)."""
    S, T = sup.num_sequences, sup.frames_per_sequence
    times = np.full(sup.num_states, -1, np.int64)
    times[0] = 0
    src = np.repeat(np.arange(sup.num_states), np.diff(sup.arc_begin))
    for a in range(len(src)):  # (arcs are state-major and the states time-sorted: a source's time is known by now)
        times[sup.nextstate[a]] = times[src[a]] + 1
    tau = times[src]
    assert tau.min() == 0 and tau.max() == S * T - 1
    mask = np.zeros((S * T, sup.label_dim), bool)
    mask[(tau % T) * S + tau // T, np.asarray(sup.ilabel) - 1] = True
    return mask


def unused_pdfs(fst):
    """Columns that no arc of the graph carries."""
    used = np.zeros(fst.num_pdfs, bool)
    used[np.asarray(fst.ilabel) - 1] = True
    return np.flatnonzero(~used)


def bad_value_picks(family):
    """About ten (t, s, c) positions for one bad element: every t of {0, 1, M-1, M, M+1, T-1} (the prologue's row, the first
    loop frame, both sides of the meeting frame M = T // 2, the epilogue's row), both of s in {0, S-1} and of c in {0, P-1},
    one column in every further plane of 4096 pdfs, the first column of a ragged last float4 (P % 4 != 0), and on the graph
    with unused pdfs nothing but columns no arc carries."""
    fst = den_fst(family.graph)
    S, T, P = family.S, family.T, fst.num_pdfs
    M = T // 2
    frames = sorted({0, 1, M - 1, M, M + 1, T - 1})
    if family.graph == "unused":
        cols = unused_pdfs(fst)
        frames += [M, T - 1, 0, 1]
        return sorted({(t, (0, S - 1)[i % 2], int(cols[(i * 7) % len(cols)])) for i, t in enumerate(frames)})
    picks = [(t, (0, S - 1)[i % 2], (0, P - 1)[(i // 2) % 2]) for i, t in enumerate(frames)]
    picks += [(M, 0, P - 1), (T - 1, S - 1, 0), (0, S - 1, P - 1), (M - 1, S - 1, 0)]
    picks += [(M + k % 2, S - 1, 4096 * k + 5) for k in range(1, (P + 4095) // 4096) if 4096 * k + 5 < P]
    if P % 4:
        picks += [(T - 1, 0, P - P % 4), (0, S - 1, P - P % 4)]
    return sorted(set(picks))


def objective_picks(family):
    """Three of them for the whole objective: first frame, meeting frame, last frame."""
    S, T = family.S, family.T
    P = den_fst(family.graph).num_pdfs
    if family.graph == "unused":
        c = int(unused_pdfs(den_fst(family.graph))[3])
        return [(0, 0, c), (T // 2, S - 1, c), (T - 1, 0, c)]
    return [(0, 0, 0), (T // 2, S - 1, P - 1), (T - 1, S - 1, P // 2)]


# ---- rows as they lie ------------------------------------------------------------------------------------------------------
SLACK = 64  # floats behind the last row that still belong to the buffer


def strided(rows, cols, stride, offset, fill, device="cpu"):
    """(buffer, view): a flat float32 tensor of offset + rows * stride + SLACK floats filled with ``fill``, and the (rows, cols)
    matrix of row stride ``stride`` that starts ``offset`` floats into it."""
    assert stride >= cols and offset >= 0
    buffer = torch.full((offset + rows * stride + SLACK,), float(fill), dtype=torch.float32, device=device)
    view = buffer[offset:offset + rows * stride].view(rows, stride)[:, :cols]
    return buffer, view


def vector_path(view):
    """api.cpp's rule restated: the 16-byte row path is taken iff cols % 4 == 0, row_stride % 4 == 0 and the base address is
    16-byte aligned; else the four-dword one."""
    return view.shape[1] % 4 == 0 and view.stride(0) % 4 == 0 and view.data_ptr() % 16 == 0


def outside(buffer, view):
    """The buffer's floats that are not the view's, as int32 bit patterns (in front of the offset, between the rows, behind
    the last row)."""
    off = (view.data_ptr() - buffer.data_ptr()) // 4
    rows, cols = view.shape
    inside = torch.zeros(buffer.numel(), dtype=torch.bool, device=buffer.device)
    inside[off:off + rows * view.stride(0)].view(rows, view.stride(0))[:, :cols] = True
    return buffer.view(torch.int32)[~inside]


def row_variants(P):
    """name -> ((y_stride, y_offset, d_stride, d_offset), expected (y_vec, d_vec))"""
    return {
        "padded_both_vector": ((P + 4, 0, P + 4, 0), (True, True)),
        "y_scalar_d_vector": ((P + 3, 0, P, 0), (False, True)),
        "y_vector_d_scalar": ((P, 0, P + 1, 0), (True, False)),
        "odd_bases_both_scalar": ((P + 4, 1, P + 4, 3), (False, False)),   # bases 4 and 12 bytes off
    }


# (stride - P, offset) of y, deriv and xent_deriv, drawn independently from the variants above; both states of x_vec against
# both of d_vec.  name -> (three placements, expected (y_vec, d_vec, x_vec))
OBJECTIVE_PLACEMENTS = {
    "all_vector": (((4, 0), (4, 0), (4, 0)), (True, True, True)),
    "d_vector_x_scalar_stride": (((3, 0), (0, 0), (1, 0)), (False, True, False)),
    "d_scalar_x_vector": (((0, 0), (1, 0), (4, 0)), (True, False, True)),
    "all_scalar_bases": (((4, 1), (4, 3), (4, 1)), (False, False, False)),
    "d_vector_x_scalar_base": (((4, 0), (0, 0), (4, 3)), (True, True, False)),
    "d_scalar_base_x_vector": (((1, 0), (4, 3), (0, 0)), (False, False, True)),
}

MODES = {  # name -> (accumulate, l2_scale, what the derivative's view holds before the call)
    "write": (False, 0.0, 7.0),
    "write_l2": (False, 1e-3, 7.0),
    "accumulate": (True, 0.0, 0.25),
}
SENTINEL = 7.0
