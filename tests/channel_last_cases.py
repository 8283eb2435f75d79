"""What the channel-last tests share (tests/test_channel_last_host.py, tests/test_gpu_channel_last.py): the views a model that
produces its channels last hands to ``chain_loss`` -- each a ``(B, C, T)`` view of a leaf in another layout -- and the numpy
statement of the row gather and scatter of ``tc_rows_gather`` / ``tc_rows_scatter`` as include/torchain_hip.h defines them."""
import numpy as np
import torch

import out_of_range_cases as oor

# (P, B, T): 16-byte paths for every dtype | float32 rows 16-byte aligned, 16-bit rows 8-byte only, odd B and T | scalar, B = 1
# | scalar, odd B and T
SHAPES = [(24, 2, 6), (20, 3, 5), (21, 1, 4), (21, 3, 5)]
# the leaf's layout -> how a (B, T, P) block of values sits in it
VIEWS = ("dense", "head_lo", "head_hi", "batch_pad", "time_major", "time_major_pad")
TIME_MAJOR = ("time_major", "time_major_pad")
# the pairs (input, xent_input) of one step: two leaves of one layout, or the two halves of ONE joint-head leaf either way round
PAIRS = ("dense", "head", "head_swapped", "batch_pad", "time_major", "time_major_pad")


def leaf_shape(kind, B, T, P):
    return {"dense": (B, T, P), "head_lo": (B, T, 2 * P), "head_hi": (B, T, 2 * P), "batch_pad": (B, T + 2, P),
            "time_major": (T, B, P), "time_major_pad": (T, B, P + 3)}[kind]


def region(kind, leaf, P):
    """The (B, C, T) view of a tensor in the leaf's layout (the leaf itself, its gradient, a numpy array of that shape)."""
    tr = (lambda a: a.transpose(0, 2, 1)) if isinstance(leaf, np.ndarray) else (lambda a: a.transpose(1, 2))
    tm = (lambda a: a.transpose(1, 2, 0)) if isinstance(leaf, np.ndarray) else (lambda a: a.permute(1, 2, 0))
    if kind == "dense":
        return tr(leaf)
    if kind == "head_lo":
        return tr(leaf[..., :P])
    if kind == "head_hi":
        return tr(leaf[..., P:])
    if kind == "batch_pad":
        return tr(leaf[:, :leaf.shape[1] - 2])
    if kind == "time_major":
        return tm(leaf)
    assert kind == "time_major_pad", kind
    return tm(leaf[..., :P])


def make_leaf(kind, rows, B, T, device, dtype, fill=0.25):
    """A leaf (requires grad) in the layout ``kind`` whose view holds the frame-major ``rows`` ((T*B, P) float32, row
    t*B + b); everything outside the view is ``fill``."""
    P = rows.shape[1]
    leaf = torch.full(leaf_shape(kind, B, T, P), fill, dtype=dtype, device=device)
    bct = torch.as_tensor(rows).reshape(T, B, P).permute(1, 2, 0).to(device).to(dtype)
    region(kind, leaf, P).copy_(bct)
    return leaf.requires_grad_(True)


# ---- numpy statements ---------------------------------------------------------------------------------------------------
def gather_np(flat, offset, B, T, P, sb, st, out_stride, sentinel):
    """tc_rows_gather: out2d[(t*B + b) * out_stride + c] = (float) in[offset + b*sb + t*st + c]; the padding columns keep the
    sentinel.  ``flat``: the storage as a 1-D float32 array (16-bit values widened, which is exact)."""
    out = np.full((T * B, out_stride), sentinel, np.float32)
    for t in range(T):
        for b in range(B):
            at = offset + (b * sb if B > 1 else 0) + (t * st if T > 1 else 0)
            out[t * B + b, :P] = flat[at:at + P]
    return out


def scatter_np(in2d, B, T, P, scale, w=None, c=0.0, y_btp=None):
    """tc_rows_scatter in float32, before the one rounding of a 16-bit tensor: (B, T, P) from ``in2d[(t*B + b), :P]``.
    Plain: fl32(scale * v).  Weights: fl32(fl32(scale * w[row]) * v), one multiply of v.  Penalty (``y_btp``: the network
    output in (B, T, P)): fl32(w[row] * g') with g' = out_of_range_cases.penalized(fl32(scale * v), y, c)."""
    v = np.asarray(in2d, np.float32)[:, :P].reshape(T, B, P).transpose(1, 0, 2)
    scale = np.float32(scale)
    wf = None if w is None else np.asarray(w, np.float32).reshape(T, B).T[:, :, None]
    with np.errstate(invalid="ignore", over="ignore"):
        if c > 0.0:
            g = oor.penalized((scale * v).astype(np.float32), y_btp, c)
            return g if wf is None else (wf * g).astype(np.float32)
        if wf is not None:
            return ((scale * wf).astype(np.float32) * v).astype(np.float32)
        return (scale * v).astype(np.float32)
