"""Writer of end-to-end chain egs: ``<Supervision>`` with ``<End2End>`` true, then ``<Fsts>``, one OpenFst
``compact_acceptor`` per sequence (each with its own start state), ``</Fsts>``, the optional ``<AlignmentPdfs>`` and
``</Supervision>`` -- [K] ``Supervision::Write`` restated from the published chain-supervision.cc, as the readers
(csrc/egs_reader.cpp, torchain_amd/egs.py) read it.  Inputs, indexes and deriv weights are written by
tests/kaldi_egs_writer.py's helpers."""
import struct

import numpy as np

import kaldi_egs_writer as kw
from torchain_amd.egs import E2eSup


def compact_acceptor(fst):
    """One per-sequence FST ``(start, arc_begin, ilabel, arc_weight, nextstate, final)`` as a compact acceptor whose
    header carries its start state."""
    start, ab, il, aw, nx, fin = fst
    n = len(fin)

    def s(b):
        return struct.pack("<i", len(b)) + b
    elems, offs = [], [0]
    for st in range(n):
        if not np.isinf(fin[st]):
            elems.append((-1, float(fin[st]), -1))
        for a in range(ab[st], ab[st + 1]):
            elems.append((int(il[a]), float(aw[a]), int(nx[a])))
        offs.append(len(elems))
    out = struct.pack("<i", 2125659606) + s(b"compact_acceptor") + s(b"standard")
    out += struct.pack("<iiQqqq", 2, 0, 0x0000000000010000, int(start), n, int(ab[-1]))
    out += np.asarray(offs, np.uint32).tobytes()
    for (lab, w, nxt) in elems:
        out += struct.pack("<ifi", lab, w, nxt)
    return out


def supervision(sup, alignment_pdfs=None):
    out = kw._tok("<Supervision>") + kw._tok("<Weight>") + kw._basic("f", sup.weight)
    out += kw._tok("<NumSequences>") + kw._basic("i", sup.num_sequences)
    out += kw._tok("<FramesPerSeq>") + kw._basic("i", sup.frames_per_sequence)
    out += kw._tok("<LabelDim>") + kw._basic("i", sup.label_dim)
    out += kw._tok("<End2End>") + b"T "
    out += kw._tok("<Fsts>") + b"".join(compact_acceptor(f) for f in sup.fsts) + kw._tok("</Fsts>")
    if alignment_pdfs is not None:
        a = np.asarray(alignment_pdfs, np.int32)
        out += kw._tok("<AlignmentPdfs>") + bytes([4]) + struct.pack("<i", len(a)) + a.tobytes()
    return out + kw._tok("</Supervision>")


def chain_example(eg, matrix_kind="FM", alignment_pdfs=False):
    out = kw._tok("<Nnet3ChainEg>") + kw._tok("<NumInputs>") + kw._basic("i", len(eg["inputs"]))
    for io_ in eg["inputs"]:
        out += kw._tok("<NnetIo>") + kw._tok(io_["name"]) + kw.index_vector(io_["indexes"])
        out += kw.general_matrix(io_["features"], matrix_kind) + kw._tok("</NnetIo>")
    out += kw._tok("<NumOutputs>") + kw._basic("i", len(eg["outputs"]))
    for o in eg["outputs"]:
        sup = o["supervision"]
        ali = np.arange(sup.num_sequences * sup.frames_per_sequence) % sup.label_dim if alignment_pdfs else None
        out += kw._tok("<NnetChainSup>") + kw._tok(o["name"]) + kw.index_vector(o["indexes"]) + supervision(sup, ali)
        out += kw._tok("<DW2>") + kw._tok("FV") + kw._basic("i", len(o["deriv_weights"]))
        out += np.asarray(o["deriv_weights"], np.float32).tobytes() + kw._tok("</NnetChainSup>")
    return out + kw._tok("</Nnet3ChainEg>")


def write_ark(path, keyed_examples, scp_path=None, len_path=None, **kwargs):
    lines = []
    with open(path, "wb") as f:
        for key, eg in keyed_examples:
            f.write(key.encode() + b" ")
            lines.append("%s %s:%d\n" % (key, path, f.tell()))
            f.write(b"\0B" + chain_example(eg, **kwargs))
    if scp_path:
        with open(scp_path, "w") as f:
            f.writelines(lines)
    if len_path:
        with open(len_path, "w") as f:
            f.writelines("%s %d\n" % (k, eg["outputs"][0]["supervision"].frames_per_sequence) for k, eg in keyed_examples)


def example(fst, T, P, feat_dim, seed, weight=1.0, emb=None):
    """One e2e eg of one sequence: features along a random walk of T arcs through ``fst`` (the pdf's embedding + noise,
    so that a model can learn the numerator's pdfs), the FST as its supervision."""
    rng = np.random.default_rng(seed)
    start, ab, il, _aw, nx, _fin = fst
    emb = rng.standard_normal((P, feat_dim)) if emb is None else emb
    feats = 0.3 * rng.standard_normal((T, feat_dim))
    s = start if 0 <= start < len(_fin) else 0  # (an out-of-range start is written as given: the readers refuse it)
    for t in range(T):
        arcs = np.arange(ab[s], ab[s + 1])
        if len(arcs) == 0:
            break
        a = int(rng.choice(arcs))
        feats[t] += emb[il[a] - 1]
        s = int(nx[a])
    sup = E2eSup(weight, 1, T, P, [fst])
    return dict(inputs=[dict(name="input", indexes=np.array([(0, t, 0) for t in range(T)], np.int32),
                             features=feats.astype(np.float32))],
                outputs=[dict(name="output", indexes=np.array([(0, t, 0) for t in range(T)], np.int32), supervision=sup,
                              deriv_weights=np.ones(T, np.float32))])
