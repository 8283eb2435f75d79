"""Plain Python / numpy statements of what ``csrc/path_edit_kernels.hip`` computes (``include/torchain_hip.h`` has the
rules): the tokens of a frame-level pdf path, the textbook two-row Levenshtein distance, and the gradient of
``functions.sampled_risk_surrogate`` summed in double in sample order and rounded once."""
import numpy as np


def tokens_of(pdfs, token_of_pdf, starts=None):
    """The hypothesis of one path (its valid frames only), or ``None`` for a failed path: a pdf outside ``0 .. P - 1``."""
    P = len(token_of_pdf)
    out, before = [], None
    for t, q in enumerate(int(v) for v in pdfs):
        if q < 0 or q >= P:
            return None
        c = int(token_of_pdf[q])
        if starts is None:
            emit = c >= 0 and (t == 0 or c != before)
        else:
            emit = c >= 0 and int(starts[q]) != 0
        if emit:
            out.append(c)
        before = c
    return out


def levenshtein(h, r):
    """Unit-cost edit distance of two sequences of integers, two rows of the table at a time."""
    prev = list(range(len(r) + 1))
    for i, a in enumerate(h, 1):
        cur = [i] + [0] * len(r)
        for j, b in enumerate(r, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a != b))
        prev = cur
    return prev[len(r)]


def batch(pdfs, token_of_pdf, refs, ref_lengths, starts=None, frames=None):
    """``(dist, lengths, tokens)`` of ``pdfs`` ``(B, K, T)``, int32 arrays as the kernel writes them."""
    pdfs = np.asarray(pdfs)
    B, K, T = pdfs.shape
    dist = np.full((B, K), -1, np.int32)
    lens = np.full((B, K), -1, np.int32)
    tokens = np.full((B, K, T), -1, np.int32)
    for b in range(B):
        n = T if frames is None else int(frames[b])
        ref = [] if refs is None else [int(v) for v in refs[b][:int(ref_lengths[b])]]
        for k in range(K):
            h = tokens_of(pdfs[b, k, :n], token_of_pdf, starts)
            if h is None:
                continue
            lens[b, k] = len(h)
            tokens[b, k, :len(h)] = h
            dist[b, k] = levenshtein(h, ref)
    return dist, lens, tokens


def round_bfloat16(x):
    """float64 -> the nearest bfloat16 value (ties to even, one rounding), returned as float32 (exact)."""
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)  # |x| = m * 2^e, m in [0.5, 1)
    q = np.maximum(e - 1, -126) - 7  # the exponent of the last kept bit: 8 significant bits, subnormals below 2^-126
    y = np.ldexp(np.rint(np.ldexp(x, -q)), q)
    y = np.where(np.abs(y) >= 2.0 ** 128, np.copysign(np.inf, x), y)
    return np.where(np.isfinite(x), y, x).astype(np.float32)


def round_to(x, dtype):
    """float64 -> ``dtype`` (``"float32"``, ``"float16"``, ``"bfloat16"``) in one rounding, as a numpy array that holds the
    value exactly (bfloat16: float32)."""
    if dtype == "bfloat16":
        return round_bfloat16(x)
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype({"float32": np.float32, "float16": np.float16}[dtype])


def risk_weights(risks):
    """``(r - mean_k r) / (K - 1)`` in float64.  With integer risks and K a power of two the mean is exact however it is
    formed, and so are these."""
    r = np.asarray(risks, np.float64)
    return (r - r.mean(axis=1, keepdims=True)) / (r.shape[1] - 1)


def risk_grad(y, pdfs, weight, grad_output, dtype, frames=None):
    """The gradient of ``sum_s grad_output[s] * L_s`` in ``y`` ``(B, C, T)`` (float64 holding the input's values exactly):
    per (s, pdf, t) the double sum, in sample order, of ``grad_output[s] * weight[s][k]`` over the samples that have that pdf
    at ``t``, where the pdf is valid and ``-30 <= y <= 30``; rounded once to ``dtype``; ``+0`` elsewhere."""
    y = np.asarray(y, np.float64)
    pdfs = np.asarray(pdfs)
    B, C, T = y.shape
    K = pdfs.shape[1]
    weight = np.asarray(weight, np.float64)
    acc = np.zeros((B, C, T), np.float64)
    for s in range(B):
        n = T if frames is None else int(frames[s])
        for t in range(n):
            for k in range(K):
                q = int(pdfs[s, k, t])
                if 0 <= q < C and -30.0 <= y[s, q, t] <= 30.0:
                    acc[s, q, t] = acc[s, q, t] + np.float64(grad_output[s]) * weight[s, k]
    return round_to(acc, dtype)
