"""What the out-of-range tests share (tests/test_out_of_range_host.py, tests/test_gpu_out_of_range.py): the numpy float32
statement of the penalty exactly as include/torchain_hip.h defines it for ``tc_chain_step_penalized``, and the seeded inputs
-- N(0, 1) network outputs of which a fixed share is overwritten with ``+-(30 + U(0.5, 20))``."""
import numpy as np

from torchain_amd import synth

LIMIT = np.float32(30.0)
KINDS = ("none", "sparse", "dense", "edge")
# (graph, S, T, paths) of the two small workloads the GPU tests run their whole matrix on
SMALL = dict(fst=(40, 4, 20, 6), S=2, T=6)
MEDIUM = dict(fst=(700, 5, 300, 19), S=4, T=30)
# a second tile of the (B, C, T) copy back along the frames (240 a tile) and along the channels (64 a tile); the leftover is
# one frame (element-wise stores), two (4-byte stores) and four (8-byte stores of a 16-bit tensor)
TILED = {T: dict(fst=(120, 4, 72, 6), S=2, T=T) for T in (241, 242, 244)}


def excess(y):
    """p: the part of ``y`` beyond +-LIMIT, one float32 subtract; 0 inside the range and for NaN and +-inf."""
    y = np.asarray(y, np.float32)
    with np.errstate(invalid="ignore"):
        p = np.where(y > LIMIT, y - LIMIT, np.where(y < -LIMIT, y + LIMIT, np.float32(0.0))).astype(np.float32)
    p[~np.isfinite(y)] = 0.0
    return p


def term(y, c):
    """t = fl32(fl32(2 * c) * p): one float32 multiply."""
    c2 = np.float32(2.0) * np.float32(c)
    with np.errstate(over="ignore"):
        return (c2 * excess(y)).astype(np.float32)


def penalized(g, y, c):
    """g' = fl32(g + t); an element with p == 0 keeps g's bits (a zero's sign included)."""
    g = np.asarray(g, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(excess(y) != 0, (g + term(y, c)).astype(np.float32), g)


def overwrite(y, kind, seed=7):
    """A copy of the (rows, cols) outputs ``y`` with the kind's share of elements out of range (drawn from
    ``default_rng(seed)``): ``none``; ``sparse``: about 1 % of the elements; ``dense``: every element of 3 whole rows;
    ``edge``: the sparse mask and signs, at exactly +-30 (so p = 0 everywhere).  Returns (y, number out of range)."""
    assert kind in KINDS, kind
    y = np.array(y, np.float32)
    rng = np.random.default_rng(seed)
    mask = rng.random(y.shape, dtype=np.float32) < 0.01
    if not mask.any():
        mask.flat[rng.integers(y.size)] = True
    sign = np.where(rng.random(y.shape, dtype=np.float32) < 0.5, np.float32(-1.0), np.float32(1.0))
    mag = np.float32(30.5) + np.float32(19.5) * rng.random(y.shape, dtype=np.float32)  # 30 + U(0.5, 20)
    rows = rng.choice(y.shape[0], size=3, replace=False)
    if kind == "sparse":
        y[mask] = (sign * mag)[mask]
    elif kind == "edge":
        y[mask] = (sign * LIMIT)[mask]
    elif kind == "dense":
        y[rows] = (sign * mag)[rows]
    return y, int((np.abs(y) > LIMIT).sum())


def workload(spec, kind, seed=1):
    """(fst, synth supervision, (S*T, P) outputs, number out of range) of one of the small workloads above."""
    states, degree, pdfs, fseed = spec["fst"]
    S, T = spec["S"], spec["T"]
    fst = synth.random_den_fst(states, degree, pdfs, seed=fseed)
    sup = synth.random_supervision(fst, S, T, 2, seed=seed)
    y, n = overwrite(synth.random_nnet_output(S, T, pdfs, seed=seed), kind)
    return fst, sup, y, n


def took_soft_failure(objf, weight):
    """The step's soft-failure route leaves objf = -10 * weight (or something that is not finite)."""
    return not np.isfinite(objf) or objf == -10.0 * weight
