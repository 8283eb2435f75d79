"""Handles of the chain loss: mirrors ``torchain/io.py`` of the reference for the hot path.

``DenominatorGraph`` (reference ``io.py:51-57``) and ``Supervision`` (``io.py:20-31``) keep the
attributes the reference exposes (``.ptr``, ``.n_pdf``, ``.n_batch``, ``.n_frame``, ``.shape``) but
wrap the C-ABI handles of libtorchain_hip.so instead of heap Kaldi objects.  The Kaldi egs readers
of the reference (``Example``, ``RandExample``, ``open_example``, ``print_key_length``, ``io.py:60-175``) are
here too, on top of ``torchain_amd.egs`` (a Kaldi-free parser of the ``<Nnet3ChainEg>`` formats).
"""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor
from contextlib import contextmanager

import numpy as np
import torch

from . import egs as _egs
from ._lib import check, lib


def _tuning_cache_path():
    return os.environ.get("TORCHAIN_TUNING_CACHE") or os.path.join(os.path.expanduser("~"), ".cache", "torchain_amd", "tuning.json")


def set_kaldi_device(device_id=0):
    """Reference ``io.py:15-17`` re-points Kaldi's process-wide CuDevice singleton at a torch
    device.  The HIP path is stateless (device and stream are explicit arguments of every call), so
    this only selects the current torch device, which is what callers rely on afterwards."""
    if torch.cuda.is_available():
        torch.cuda.set_device(device_id)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _concat_fsts(fsts, e2e, who):
    """The per-sequence CSR tuples of ``from_fsts`` (``e2e`` false) / ``from_e2e_fsts`` as the concatenated arrays the C
    ABI takes: ``(seq_state_begin, start, arc_begin, ilabel, arc_weight, nextstate, final)``."""
    seq_begin, starts, ab, il, aw, nx, fin = [0], [], [np.zeros(1, np.int32)], [], [], [], []
    arcs = 0
    for i, f in enumerate(fsts):
        if len(f) != (6 if e2e else 5):
            raise ValueError("%s: sequence %d: an FST is a tuple of %d arrays" % (who, i, 6 if e2e else 5))
        start, (arc_begin, ilabel, arc_weight, nextstate, final) = (f[0], f[1:]) if e2e else (0, f)
        arc_begin = np.asarray(arc_begin, dtype=np.int64)
        final = np.asarray(final, dtype=np.float32).ravel()
        if arc_begin.shape != (len(final) + 1,) or arc_begin[0] != 0:
            raise ValueError("%s: sequence %d: arc_begin must have len(final) + 1 entries starting at 0" % (who, i))
        if any(np.asarray(x).size != arc_begin[-1] for x in (ilabel, arc_weight, nextstate)):
            raise ValueError("%s: sequence %d: ilabel, arc_weight and nextstate must have arc_begin[-1] entries" % (who, i))
        seq_begin.append(seq_begin[-1] + len(final))
        starts.append(int(start))
        ab.append((arc_begin[1:] + arcs).astype(np.int32))
        arcs += int(arc_begin[-1])
        il.append(np.asarray(ilabel, dtype=np.int32).ravel())
        aw.append(np.asarray(arc_weight, dtype=np.float32).ravel())
        nx.append(np.asarray(nextstate, dtype=np.int32).ravel())
        fin.append(final)
    return (_i32(seq_begin), _i32(starts), _i32(np.concatenate(ab)), _i32(np.concatenate(il)), _f32(np.concatenate(aw)),
            _i32(np.concatenate(nx)), _f32(np.concatenate(fin)))


def _normalized(who, den_graph, fsts, e2e, scale, label_dim):
    """``fsts`` composed with ``den_graph``'s normalization acceptor for a constructor: an empty or oversized product is
    an error that names the sequences."""
    out, info = den_graph._normalize(fsts, e2e, scale, 200000, label_dim, who)
    bad = [i for i, f in enumerate(out) if f is None]
    if bad:
        empty = [i for i in bad if info["status"][i] == 1]
        raise ValueError("%s: sequences %s have no path in the denominator graph%s" % (who, empty, "" if empty == bad else
                         "; sequences %s exceed %d states once composed" % ([i for i in bad if i not in empty], 200000)))
    return out


class DenominatorGraph:
    """``DenominatorGraph(rspec, n_pdf)`` as in the reference (``io.py:51-54`` ->
    ``my_lib_denominator_graph_new``, ``src/my_lib_example.cpp:129-134``): ``rspec`` is the path of an
    OpenFst ``den.fst``.  ``rspec`` may also be an in-memory FST: any object with the fields
    ``num_states, src, dst, ilabel, weight, final, start`` (``torchain_amd.synth.DenFst``)."""

    def __init__(self, rspec, n_pdf):
        self.rspec = rspec
        self.n_pdf = int(n_pdf)
        handle = C.c_void_p()
        if isinstance(rspec, (str, bytes)):
            path = rspec.encode() if isinstance(rspec, str) else rspec
            check(lib.tc_den_graph_read(C.byref(handle), path, self.n_pdf), "tc_den_graph_read(%r)" % rspec)
        else:
            f = rspec
            src, dst, il = _i32(f.src), _i32(f.dst), _i32(f.ilabel)
            w, fin = _f32(f.weight), _f32(f.final)
            check(lib.tc_den_graph_create(C.byref(handle), int(f.num_states), len(src), _p(src), _p(dst), _p(il),
                                          _p(w), _p(fin), int(f.start), self.n_pdf), "tc_den_graph_create")
        self.ptr = handle

    def __del__(self, _free=lib.tc_den_graph_free):
        ptr = getattr(self, "ptr", None)
        if ptr:
            _free(ptr)
            self.ptr = None

    @property
    def num_states(self):
        return lib.tc_den_graph_num_states(self.ptr)

    @property
    def num_arcs(self):
        return lib.tc_den_graph_num_arcs(self.ptr)

    def initial_probs(self):
        out = np.zeros(self.num_states, np.float32)
        check(lib.tc_den_graph_initial_probs(self.ptr, _p(out)), "tc_den_graph_initial_probs")
        return out

    def prepare(self, device=None, variant=None):
        """Uploads the immutable tables to ``device`` now instead of on the first loss call, and settles which of the
        graph's two kernels batches above one sequence per two CUs run there (``tc_den_graph_tuning``): ``variant``
        (0 fused / 1 two-sequence) if given -- ``parallel.sync_den_graph_variant`` passes rank 0's --, else the choice
        an earlier run measured for this graph on this kind of device (a JSON cache: ``$TORCHAIN_TUNING_CACHE`` or
        ``~/.cache/torchain_amd/tuning.json``, keyed by ``tc_den_graph_hash`` and the device name), else the library
        times the two kernels once and the result goes into that cache.  So the choice -- and with it the last bits of
        the results -- is the same from run to run and from rank to rank.  Since round 5 the cache is the LIBRARY's
        (``csrc/tuning_cache.cpp``, inside ``tc_den_graph_prepare``): a caller of the C ABI gets the same without this
        class."""
        dev = torch.cuda.current_device() if device is None else torch.device(device).index
        dev = int(dev or 0)
        done = self.__dict__.setdefault("_prepared", {})
        if dev in done and variant is None:
            return self
        if variant is not None:
            check(lib.tc_den_graph_set_variant(self.ptr, dev, int(variant)), "tc_den_graph_set_variant")
        check(lib.tc_den_graph_prepare(self.ptr, dev), "tc_den_graph_prepare")  # (looks the graph up in the cache, or times)
        done[dev] = True
        return self

    def stats(self):
        out = np.zeros(9, np.int64)
        check(lib.tc_den_graph_stats(self.ptr, _p(out)), "tc_den_graph_stats")
        keys = ("fwd_slots", "bwd_slots", "lds_bytes", "threads", "fwd_rows", "bwd_rows", "fwd_conflict_x1000",
                "bwd_conflict_x1000", "tied")
        return dict(zip(keys, (int(x) for x in out)))


    def tuning(self, device):
        """Which kernel batches above one sequence per two CUs run on ``device`` (``tc_den_graph_tuning``) and the
        two times the choice was made on."""
        import ctypes as C
        dev = device if isinstance(device, int) else torch.device(device).index
        choice, a, b = C.c_int32(0), C.c_float(0), C.c_float(0)
        check(lib.tc_den_graph_tuning(self.ptr, int(dev or 0), C.byref(choice), C.byref(a), C.byref(b)),
              "tc_den_graph_tuning")
        return {"two_sequence_kernel": int(choice.value), "fused_ms": float(a.value), "two_sequence_ms": float(b.value)}

    def debug_walk(self, direction, gather, pdf_factor):
        """Diagnostic (host only): replays one arc walk from the built schedules, see
        ``tc_den_graph_debug_walk``.  Used by the CPU tests of the schedule builder."""
        gather = np.ascontiguousarray(gather, np.float32)
        pdf_factor = np.ascontiguousarray(pdf_factor, np.float32)
        out = np.zeros(lib.tc_den_graph_num_states(self.ptr), np.float32)
        check(lib.tc_den_graph_debug_walk(self.ptr, int(direction), _p(gather), _p(pdf_factor), _p(out)),
              "tc_den_graph_debug_walk")
        return out

    def arcs(self):
        """The graph's arcs as the handle keeps them (``tc_den_graph_arcs``): ``(src, dst, pdf, prob)``, ``pdf`` 0-based,
        ``prob`` the float32 probabilities the denominator kernels use."""
        n = self.num_arcs
        src, dst, pdf, prob = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        check(lib.tc_den_graph_arcs(self.ptr, _p(src), _p(dst), _p(pdf), _p(prob)), "tc_den_graph_arcs")
        return src, dst, pdf, prob

    def normalize_fsts(self, fsts, e2e=False, scale=1.0, max_states=200000):
        """Puts this graph's weights on supervisions the caller built (``tc_den_compose``): every FST composed with the
        graph's normalization acceptor, as [K] ``AddWeightToSupervisionFst`` does to every supervision Kaldi writes into an
        eg.  A path the graph does not contain is gone, one it contains gains ``scale * (-log pi(h_0) - sum log w)`` (summed
        over the start states and parallel arcs that admit it: nothing is determinised), so the objective of the result is
        bounded by 0.  ``scale``: [K] e2e ``normalization_fst_scale``; 0 only restricts the paths.

        ``fsts``: per-sequence tuples as ``Supervision.from_fsts`` (``e2e`` false) or ``from_e2e_fsts`` takes them.  Returns
        ``(fsts_out, info)``: ``fsts_out`` in the same form -- start state 0, states in breadth-first order, so a
        time-unfolded input stays in time order -- with ``None`` for a sequence whose product is empty or has more than
        ``max_states`` states before trimming; ``info``: per-sequence numpy arrays ``status`` (0, 1 = empty, 2 = too large),
        ``states_in``, ``arcs_in``, ``states_out``, ``arcs_out``.  Composed end-to-end FSTs can exceed the end-to-end
        numerator's 2048 states / 8192 arcs, composed regular ones can move to the level-windowed numerator: ``info`` and
        ``Supervision.stats()`` say so before anything runs.  Host only: no GPU is touched and the graph is not modified."""
        return self._normalize(fsts, e2e, scale, max_states, self.n_pdf, "normalize_fsts")

    def _normalize(self, fsts, e2e, scale, max_states, label_dim, who):
        fsts = list(fsts)
        if not fsts:
            raise ValueError("%s: no FSTs" % who)
        scale = float(scale)
        if not (scale >= 0.0) or scale == float("inf"):
            raise ValueError("%s: the normalization scale must be finite and >= 0, got %r" % (who, scale))
        if int(max_states) < 1:
            raise ValueError("%s: max_states must be at least 1" % who)
        sb, st, ab, il, aw, nx, fin = _concat_fsts(fsts, bool(e2e), who)
        res = C.c_void_p()
        check(lib.tc_den_compose(C.byref(res), self.ptr, len(fsts), int(label_dim), int(bool(e2e)), _p(sb), _p(st), _p(ab), _p(il),
                                 _p(aw), _p(nx), _p(fin), scale, int(max_states)), "tc_den_compose")
        try:
            S = len(fsts)
            sizes = np.zeros(3, np.int64)
            check(lib.tc_den_compose_sizes(res, _p(sizes)), "tc_den_compose_sizes")
            ns, na = int(sizes[1]), int(sizes[2])
            status, info4 = np.zeros(S, np.int32), np.zeros((S, 4), np.int64)
            check(lib.tc_den_compose_info(res, _p(status), _p(info4)), "tc_den_compose_info")
            osb, ost, oab = np.zeros(S + 1, np.int32), np.zeros(S, np.int32), np.zeros(ns + 1, np.int32)
            oil, onx = np.zeros(na, np.int32), np.zeros(na, np.int32)
            oaw, ofin = np.zeros(na, np.float32), np.zeros(ns, np.float32)
            check(lib.tc_den_compose_copy(res, _p(osb), _p(ost), _p(oab), _p(oil), _p(oaw), _p(onx), _p(ofin)), "tc_den_compose_copy")
        finally:
            lib.tc_den_compose_free(res)
        out = []
        for s in range(S):
            if status[s] != 0:
                out.append(None)
                continue
            s0, s1 = int(osb[s]), int(osb[s + 1])
            a0, a1 = int(oab[s0]), int(oab[s1])
            f = (oab[s0:s1 + 1] - a0, oil[a0:a1].copy(), oaw[a0:a1].copy(), onx[a0:a1].copy(), ofin[s0:s1].copy())
            out.append(((int(ost[s]),) + f) if e2e else f)
        info = {"status": status, "states_in": info4[:, 0].copy(), "arcs_in": info4[:, 1].copy(),
                "states_out": info4[:, 2].copy(), "arcs_out": info4[:, 3].copy()}
        return out, info

    def best_path(self, nnet_output, frames=None, return_states=False, max_workspace_bytes=1 << 30, workspace=None, out=None,
                  n_batch=None):
        """The single strongest path through this graph under ``nnet_output`` (``tc_den_best_path``): a phone-LM-constrained
        free decoding of every sequence, the denominator's counterpart of ``Supervision.best_path``.  A path's score is
        ``log pi(h_0) + sum_t (log w(a_t) + y_{t-1}(pdf(a_t)))`` with the graph's initial probabilities, every state final at
        cost 0 and ``y`` as it is (no clamp, no leaky-HMM coefficient).  Returns ``(pdfs, scores)`` or, with
        ``return_states``, ``(pdfs, scores, states)`` on the input's device: ``pdfs`` int32 ``(B, Tmax)``, 0-based, ``scores``
        float64 ``(B,)``, ``states`` int32 ``(B, Tmax + 1)`` (the FST's states); ``-1`` in padding slots.  A sequence with a
        NaN or an infinity in its valid frames gets score NaN and ``-1`` everywhere.

        ``nnet_output`` is contiguous ``(B, C, T)`` float32 / bfloat16 / float16 or 2-D float32 ``(T*B, C)`` with unit column
        stride (row ``t*B + b``); a 2-D input needs ``frames`` or ``n_batch`` to tell ``B``.  ``frames``: a list, array or
        int tensor of ``B`` lengths in ``1 .. Tmax`` (``Supervision.frames`` of a ragged handle as it is); ``None``: ``Tmax``
        each.  Shapes, dtypes and lengths are checked here, before any library call.

        The call keeps every state's score of every frame, ``(Tmax + 1) * 4 * (states rounded up to 4)`` bytes a sequence.
        When that exceeds ``max_workspace_bytes`` for the whole batch (or the size of ``workspace``, a CUDA uint8 tensor to
        reuse instead of allocating one), consecutive groups of sequences run one after the other, as few as fit, on the same
        stream into the same outputs: the bits are those of one call.  (A group of a 2-D input is gathered into a matrix of
        its own first.)  ``out``: preallocated ``(pdfs, scores)`` or ``(pdfs, scores, states)``.  Asynchronous on the current
        stream; no autograd."""
        x = nnet_output.detach() if isinstance(nnet_output, torch.Tensor) else nnet_output
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError("best_path: nnet_output must be a CUDA tensor (only the HIP implementation is available)")
        P = self.n_pdf
        dtypes = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}  # TC_DTYPE_*
        if x.dim() == 3:
            B, T = int(x.shape[0]), int(x.shape[2])
            if int(x.shape[1]) != P or B < 1 or T < 1:
                raise ValueError("best_path: nnet output of shape %s is not (B, %d, T)" % (tuple(x.shape), P))
            if x.dtype not in dtypes:
                raise TypeError("best_path: a (B, C, T) output must be float32, bfloat16 or float16, got %s" % x.dtype)
            if n_batch is not None and int(n_batch) != B:
                raise ValueError("best_path: n_batch = %d, but the output has %d sequences" % (int(n_batch), B))
        elif x.dim() == 2:
            if x.dtype != torch.float32:
                raise TypeError("best_path: a 2-D output must be float32, got %s" % x.dtype)
            if frames is None and n_batch is None:
                raise ValueError("best_path: a 2-D output needs `frames` or `n_batch` to tell the number of sequences")
            B = int(n_batch) if n_batch is not None else len(frames)
            if int(x.shape[1]) != P or B < 1 or x.shape[0] < B or x.shape[0] % B != 0:
                raise ValueError("best_path: nnet output of shape %s is not (T * %d, %d)" % (tuple(x.shape), B, P))
            T = int(x.shape[0]) // B
        else:
            raise ValueError("best_path: nnet output must be (B, C, T) or (T*B, C), got shape %s" % (tuple(x.shape),))
        lengths = None
        if frames is not None:
            lengths = frames.detach().cpu().numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)
            if lengths.ndim != 1 or lengths.dtype.kind not in "iu":
                raise TypeError("best_path: frames must be a list or an int tensor of lengths")
            if len(lengths) != B:
                raise ValueError("best_path: %d lengths for %d sequences" % (len(lengths), B))
            if lengths.min() < 1 or lengths.max() > T:
                raise ValueError("best_path: every length must be in 1 .. %d, got %d .. %d" % (T, lengths.min(), lengths.max()))
        device = x.device
        if x.dim() == 3 and not x.is_contiguous():
            x = x.contiguous()
        if x.dim() == 2 and (x.stride(1) != 1 or x.stride(0) < P):
            x = x.contiguous()
        if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8
                                      or workspace.device != device or not workspace.is_contiguous()):
            raise ValueError("best_path: workspace must be a contiguous uint8 tensor on the output's device")
        shapes = [((B, T), torch.int32), ((B,), torch.float64)] + ([((B, T + 1), torch.int32)] if return_states else [])
        if out is not None:
            if len(out) != len(shapes):
                raise ValueError("best_path: out must hold %d tensors" % len(shapes))
            for o, (shape, dt) in zip(out, shapes):
                if tuple(o.shape) != shape or o.dtype != dt or o.device != device or not o.is_contiguous():
                    raise ValueError("best_path: an out tensor is not a contiguous %s %s on %s" % (dt, shape, device))
            outs = list(out)
        else:
            outs = [torch.empty(shape, dtype=dt, device=device) for shape, dt in shapes]
        need = lambda n: int(lib.tc_den_best_path_workspace_bytes(self.ptr, n, T))  # noqa: E731  (host arithmetic only)
        cap = int(max_workspace_bytes) if workspace is None else min(int(max_workspace_bytes), workspace.numel())
        group = B
        if need(B) > cap:
            group = max(1, min(B, cap // need(1)))
            while group > 1 and need(group) > cap:
                group -= 1
            if need(group) > cap:
                raise ValueError("best_path: one sequence needs %d bytes of workspace, %d are allowed" % (need(1), cap))
        ws = workspace if workspace is not None else torch.empty(need(group), dtype=torch.uint8, device=device)
        fr = None if lengths is None else torch.from_numpy(np.ascontiguousarray(lengths, dtype=np.int32)).to(device)
        with torch.cuda.device(device):
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            for s0 in range(0, B, group):
                n = min(group, B - s0)
                if x.dim() == 3:
                    xg, stride = x[s0:s0 + n], 0
                elif n == B:
                    xg, stride = x, x.stride(0)
                else:  # rows t*B + s0 .. t*B + s0 + n - 1 of every frame, as a matrix of the group's own
                    rs = x.stride(0)
                    xg = torch.as_strided(x, (T, n, P), (B * rs, rs, 1), x.storage_offset() + s0 * rs).reshape(T * n, P)
                    stride = xg.stride(0)  # (a group of one sequence stays a view, rows B * rs apart)
                check(lib.tc_den_best_path(self.ptr, n, C.c_void_p(xg.data_ptr()), dtypes[x.dtype], int(x.dim() == 3), n * T, P,
                                           stride, None if fr is None else C.c_void_p(fr[s0:s0 + n].data_ptr()), T,
                                           C.c_void_p(outs[0][s0:s0 + n].data_ptr()),
                                           C.c_void_p(outs[2][s0:s0 + n].data_ptr()) if return_states else None,
                                           C.c_void_p(outs[1][s0:s0 + n].data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                                           device.index, stream), "tc_den_best_path")
        return tuple(outs)

    def expected_accuracy(self, nnet_output, ref_pdfs, pdf_class=None, frames=None, leaky_hmm_coefficient=1e-5, n_batch=None,
                          max_workspace_bytes=8 << 30):
        """The expected frame accuracy of this graph's paths under ``nnet_output`` against the frame-level reference
        ``ref_pdfs`` (``tc_den_expected_accuracy``): the lattice-free sMBR criterion, per sequence
        ``E[A] = sum_paths P(path | y) * sum_t a_t(pdf_t(path))`` under the denominator's own model (outputs clamped to +-30,
        the graph's initial probabilities, ``leaky_hmm_coefficient``, every state final).  ``a_t(j)`` is 1 where
        ``class(j) == class(ref_t)``, else 0.  Returns ``(acc, frame_acc)`` on the input's device: float64 ``(B,)`` and
        float32 ``(B, Tmax)``, the frames' expected accuracies (0 in padding frames), which sum to ``acc``.  A sequence with
        a NaN or an infinity in its valid frames gets NaN.

        ``nnet_output``, ``frames`` and ``n_batch`` are ``best_path``'s: contiguous ``(B, C, T)`` float32 / bfloat16 / float16
        or 2-D float32 ``(T*B, C)`` (row ``t*B + b``); anything that is not 2-D float32 is copied into such a matrix first --
        this is not a hot path.  ``ref_pdfs``: an int tensor or array ``(B, Tmax)`` of 0-based pdfs, the layout ``best_path``
        and ``Supervision.best_path`` return; a value outside ``0 .. n_pdf - 1`` (their ``-1``, or a caller's mark for
        silence) means that the frame scores nothing.  ``pdf_class``: ``None`` (state-level sMBR) or ``n_pdf`` ints, e.g. a
        pdf -> phone map for an MPFE-style criterion.  The workspace is the denominator's; beyond ``max_workspace_bytes`` a
        ``ValueError`` names the bytes (groups of sequences are not run).  Asynchronous on the current stream; no autograd:
        ``functions.den_expected_accuracy`` is the differentiable entry."""
        st = self._expected_accuracy("expected_accuracy", nnet_output, ref_pdfs, pdf_class, frames, leaky_hmm_coefficient,
                                     n_batch, max_workspace_bytes, False)
        return st["acc"], st["frame_acc"]

    def _accuracy_arguments(self, who, nnet_output, frames, n_batch):
        """The checks of the expected-accuracy entries on ``nnet_output``, ``frames`` and ``n_batch``, before any library call:
        ``(x, B, T, lengths)``, ``x`` the detached tensor and ``lengths`` a numpy array or ``None``."""
        x = nnet_output.detach() if isinstance(nnet_output, torch.Tensor) else nnet_output
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError("%s: nnet_output must be a CUDA tensor (only the HIP implementation is available)" % who)
        P = self.n_pdf
        dtypes = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}  # TC_DTYPE_*
        if x.dim() == 3:
            B, T = int(x.shape[0]), int(x.shape[2])
            if int(x.shape[1]) != P or B < 1 or T < 1:
                raise ValueError("%s: nnet output of shape %s is not (B, %d, T)" % (who, tuple(x.shape), P))
            if x.dtype not in dtypes:
                raise TypeError("%s: a (B, C, T) output must be float32, bfloat16 or float16, got %s" % (who, x.dtype))
            if n_batch is not None and int(n_batch) != B:
                raise ValueError("%s: n_batch = %d, but the output has %d sequences" % (who, int(n_batch), B))
        elif x.dim() == 2:
            if x.dtype != torch.float32:
                raise TypeError("%s: a 2-D output must be float32, got %s" % (who, x.dtype))
            if frames is None and n_batch is None:
                raise ValueError("%s: a 2-D output needs `frames` or `n_batch` to tell the number of sequences" % who)
            B = int(n_batch) if n_batch is not None else len(frames)
            if int(x.shape[1]) != P or B < 1 or x.shape[0] < B or x.shape[0] % B != 0:
                raise ValueError("%s: nnet output of shape %s is not (T * %d, %d)" % (who, tuple(x.shape), B, P))
            T = int(x.shape[0]) // B
        else:
            raise ValueError("%s: nnet output must be (B, C, T) or (T*B, C), got shape %s" % (who, tuple(x.shape)))
        lengths = None
        if frames is not None:
            lengths = frames.detach().cpu().numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)
            if lengths.ndim != 1 or lengths.dtype.kind not in "iu":
                raise TypeError("%s: frames must be a list or an int tensor of lengths" % who)
            if len(lengths) != B:
                raise ValueError("%s: %d lengths for %d sequences" % (who, len(lengths), B))
            if lengths.min() < 1 or lengths.max() > T:
                raise ValueError("%s: every length must be in 1 .. %d, got %d .. %d" % (who, T, lengths.min(), lengths.max()))
        return x, B, T, lengths

    def _accuracy_rows(self, x, B, T, stream):
        """``x`` -- ``(B, C, T)`` of float32 / bfloat16 / float16 or 2-D float32 -- as a float32 matrix ``(T*B, C)``, row
        ``t*B + b``, with unit column stride: itself, or a copy made by ``tc_rows_gather``."""
        P, device = self.n_pdf, x.device
        dtypes = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}  # TC_DTYPE_*
        if x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= P and x.data_ptr() % 4 == 0:
            return x
        # the existing gather entry: (b, t, :) rows of a channel-last tensor of `dtype` -> float32 row t*B + b
        rows = x.transpose(1, 2).contiguous() if x.dim() == 3 else x.reshape(T, B, P).transpose(0, 1).contiguous()
        y2d = torch.empty((T * B, P), dtype=torch.float32, device=device)
        check(lib.tc_rows_gather(C.c_void_p(rows.data_ptr()), dtypes[x.dtype], B, P, T, T * P, P,
                                 C.c_void_p(y2d.data_ptr()), P, device.index, stream), "tc_rows_gather")
        return y2d

    def _expected_accuracy(self, who, nnet_output, ref_pdfs, pdf_class, frames, leaky, n_batch, max_workspace_bytes, want_grad):
        """The checks, the 2-D float32 matrix and one ``tc_den_expected_accuracy`` call; returns what the gradient call needs
        beside the results.  ``want_grad``: hold the gradient's workspace against the cap as well, before anything runs."""
        x, B, T, lengths = self._accuracy_arguments(who, nnet_output, frames, n_batch)
        P = self.n_pdf
        device = x.device

        def ints(v, shape, what):
            t = v.detach() if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))
            if t.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8) or tuple(t.shape) != shape:
                raise ValueError("%s: %s must be an int tensor or array of shape %s" % (who, what, shape))
            return t.to(device=device, dtype=torch.int32).contiguous()

        ref = ints(ref_pdfs, (B, T), "ref_pdfs")
        cls = None if pdf_class is None else ints(pdf_class, (P,), "pdf_class")
        leaky = float(leaky)
        if not (0.0 <= leaky < float("inf")):
            raise ValueError("%s: the leaky-HMM coefficient must be finite and >= 0, got %r" % (who, leaky))
        need = int(lib.tc_den_expected_accuracy_workspace_bytes(self.ptr, B, T))  # (host arithmetic only)
        if want_grad:
            need = max(need, int(lib.tc_den_expected_accuracy_grad_workspace_bytes(self.ptr, B, T)))
        if need > int(max_workspace_bytes):
            raise ValueError("%s: %d sequences of %d frames need %d bytes of workspace, %d are allowed"
                             % (who, B, T, need, int(max_workspace_bytes)))
        fr = None if lengths is None else torch.from_numpy(np.ascontiguousarray(lengths, dtype=np.int32)).to(device)
        with torch.cuda.device(device):
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            y2d = self._accuracy_rows(x, B, T, stream)
            gamma = torch.empty((T * B, P), dtype=torch.float32, device=device)
            frame_acc = torch.empty((B, T), dtype=torch.float32, device=device)
            acc = torch.empty((B,), dtype=torch.float64, device=device)
            ws = torch.empty(int(lib.tc_den_expected_accuracy_workspace_bytes(self.ptr, B, T)), dtype=torch.uint8, device=device)
            check(lib.tc_den_expected_accuracy(self.ptr, B, C.c_void_p(y2d.data_ptr()), B * T, P, y2d.stride(0),
                                               None if fr is None else C.c_void_p(fr.data_ptr()), T, leaky,
                                               C.c_void_p(ref.data_ptr()), None if cls is None else C.c_void_p(cls.data_ptr()),
                                               C.c_void_p(gamma.data_ptr()), P, C.c_void_p(frame_acc.data_ptr()),
                                               C.c_void_p(acc.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(), device.index,
                                               stream), "tc_den_expected_accuracy")
        return {"acc": acc, "frame_acc": frame_acc, "y2d": y2d, "ref": ref, "cls": cls, "fr": fr, "B": B, "T": T,
                "leaky": leaky}

    def _expected_accuracy_grad(self, st, seq_scale):
        """``tc_den_expected_accuracy_grad`` on what ``_expected_accuracy`` returned: the float32 ``(T*B, C)`` gradient, each
        sequence's rows times its entry of ``seq_scale`` (float32 ``(B,)`` on the device, or ``None``)."""
        B, T, P, y2d = st["B"], st["T"], self.n_pdf, st["y2d"]
        device = y2d.device
        with torch.cuda.device(device):
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            grad = torch.empty((T * B, P), dtype=torch.float32, device=device)
            ws = torch.empty(int(lib.tc_den_expected_accuracy_grad_workspace_bytes(self.ptr, B, T)), dtype=torch.uint8, device=device)
            opt = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
            check(lib.tc_den_expected_accuracy_grad(self.ptr, B, C.c_void_p(y2d.data_ptr()), B * T, P, y2d.stride(0), opt(st["fr"]),
                                                    T, st["leaky"], C.c_void_p(st["ref"].data_ptr()), opt(st["cls"]),
                                                    C.c_void_p(st["frame_acc"].data_ptr()), opt(seq_scale),
                                                    C.c_void_p(grad.data_ptr()), P, C.c_void_p(ws.data_ptr()), ws.numel(),
                                                    device.index, stream), "tc_den_expected_accuracy_grad")
        return grad

    def expected_accuracy_dense(self, nnet_output, accuracy, frames=None, leaky_hmm_coefficient=1e-5, n_batch=None,
                                max_workspace_bytes=8 << 30, return_posteriors=False):
        """``expected_accuracy`` against SOFT references (``tc_den_expected_accuracy_dense``): ``a_t(j)`` is not the indicator of
        a reference pdf but entry ``(t, j)`` of ``accuracy``, a dense matrix held constant -- the numerator's posteriors
        (``Supervision.posteriors``: Kaldi's chain-sMBR, ``a_t(j) = gamma_num_t(j)``), label-smoothed indicators, signed
        rewards; any finite float32.  Returns ``(acc, frame_acc)``, float64 ``(B,)`` and float32 ``(B, Tmax)``, and with
        ``return_posteriors`` also the denominator posteriors ``gamma``, float32 ``(T*B, C)`` (row ``t*B + b``, +0 in padding
        rows) -- which are ``d acc[b] / d accuracy``.  A sequence with a NaN or an infinity in its valid frames of
        ``nnet_output`` or of ``accuracy`` gets NaN; the others keep their bits.  The float32 indicator of ``(ref_pdfs,
        pdf_class)`` gives the bits of ``expected_accuracy``.

        ``nnet_output``, ``frames``, ``n_batch``: as for ``expected_accuracy``.  ``accuracy`` takes the same layouts,
        independently: 2-D float32 ``(T*B, C)`` or ``(B, C, T)`` in float32 / bfloat16 / float16 (widened to float32);
        whatever is not a 2-D float32 matrix with unit column stride is copied into one.  Padding frames of either are not
        read.  Shapes and dtypes are checked before any library call.

        When the batch needs more than ``max_workspace_bytes``, consecutive groups of sequences run one after the other, as
        many at a time as fit, each on copies of its rows: the outputs are the single call's, bit for bit.  ``ValueError``
        only where one sequence alone does not fit.  Asynchronous on the current stream; no autograd:
        ``functions.den_expected_accuracy_dense`` is the differentiable entry."""
        st = self._expected_accuracy_dense("expected_accuracy_dense", nnet_output, accuracy, frames, leaky_hmm_coefficient,
                                           n_batch, max_workspace_bytes, False, return_posteriors)
        return (st["acc"], st["frame_acc"]) + ((st["gamma"],) if return_posteriors else ())

    def _expected_accuracy_dense(self, who, nnet_output, accuracy, frames, leaky, n_batch, max_workspace_bytes, want_grad,
                                 keep_gamma):
        """The checks, the two 2-D float32 matrices and ``tc_den_expected_accuracy_dense`` on every group of sequences; returns
        what the gradient call needs beside the results.  ``want_grad``: size the groups for the gradient's workspace as well.
        ``keep_gamma``: the denominator posteriors of the whole batch are part of the result."""
        x, B, T, lengths = self._accuracy_arguments(who, nnet_output, frames, n_batch)
        P, device = self.n_pdf, x.device
        a = accuracy.detach() if isinstance(accuracy, torch.Tensor) else accuracy
        if not isinstance(a, torch.Tensor) or a.device != device:
            raise ValueError("%s: accuracy must be a tensor on the output's device (%s)" % (who, device))
        if a.dim() == 3:
            if tuple(a.shape) != (B, P, T):
                raise ValueError("%s: accuracy of shape %s is not (%d, %d, %d)" % (who, tuple(a.shape), B, P, T))
            if a.dtype not in (torch.float32, torch.bfloat16, torch.float16):
                raise TypeError("%s: a (B, C, T) accuracy must be float32, bfloat16 or float16, got %s" % (who, a.dtype))
        elif a.dim() == 2:
            if tuple(a.shape) != (T * B, P):
                raise ValueError("%s: accuracy of shape %s is not (%d, %d)" % (who, tuple(a.shape), T * B, P))
            if a.dtype != torch.float32:
                raise TypeError("%s: a 2-D accuracy must be float32, got %s" % (who, a.dtype))
        else:
            raise ValueError("%s: accuracy must be (B, C, T) or (T*B, C), got shape %s" % (who, tuple(a.shape)))
        leaky = float(leaky)
        if not (0.0 <= leaky < float("inf")):
            raise ValueError("%s: the leaky-HMM coefficient must be finite and >= 0, got %r" % (who, leaky))

        def need(n):  # (host arithmetic only)
            value = int(lib.tc_den_expected_accuracy_workspace_bytes(self.ptr, n, T))
            return max(value, int(lib.tc_den_expected_accuracy_grad_workspace_bytes(self.ptr, n, T))) if want_grad else value

        cap, group = int(max_workspace_bytes), B
        if need(B) > cap:
            if need(1) > cap:
                raise ValueError("%s: one sequence of %d frames needs %d bytes of workspace, %d are allowed"
                                 % (who, T, need(1), cap))
            group = max(1, min(B, cap // need(1)))
            while need(group) > cap:
                group -= 1
            while group < B and need(group + 1) <= cap:
                group += 1
        fr = None if lengths is None else torch.from_numpy(np.ascontiguousarray(lengths, dtype=np.int32)).to(device)
        with torch.cuda.device(device):
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            y2d, a2d = self._accuracy_rows(x, B, T, stream), self._accuracy_rows(a, B, T, stream)
            frame_acc = torch.empty((B, T), dtype=torch.float32, device=device)
            acc = torch.empty((B,), dtype=torch.float64, device=device)
            gamma = torch.empty((T * B, P), dtype=torch.float32, device=device) if keep_gamma or group == B else None
            ws = torch.empty(int(lib.tc_den_expected_accuracy_workspace_bytes(self.ptr, group, T)), dtype=torch.uint8, device=device)
            for s0 in range(0, B, group):
                n = min(group, B - s0)
                yg, ag = _group_rows(y2d, s0, n, B, T), _group_rows(a2d, s0, n, B, T)
                gg = gamma if n == B else torch.empty((T * n, P), dtype=torch.float32, device=device)
                check(lib.tc_den_expected_accuracy_dense(self.ptr, n, C.c_void_p(yg.data_ptr()), n * T, P, yg.stride(0),
                                                         None if fr is None else C.c_void_p(fr[s0:s0 + n].data_ptr()), T, leaky,
                                                         C.c_void_p(ag.data_ptr()), ag.stride(0), C.c_void_p(gg.data_ptr()), P,
                                                         C.c_void_p(frame_acc[s0:s0 + n].data_ptr()),
                                                         C.c_void_p(acc[s0:s0 + n].data_ptr()), C.c_void_p(ws.data_ptr()),
                                                         ws.numel(), device.index, stream), "tc_den_expected_accuracy_dense")
                if n != B and keep_gamma:
                    gamma.view(T, B, P)[:, s0:s0 + n].copy_(gg.view(T, n, P))
        return {"acc": acc, "frame_acc": frame_acc, "gamma": gamma if keep_gamma else None, "y2d": y2d, "a2d": a2d, "fr": fr,
                "B": B, "T": T, "leaky": leaky, "group": group}

    def _expected_accuracy_dense_grad(self, st, seq_scale):
        """``tc_den_expected_accuracy_dense_grad`` on what ``_expected_accuracy_dense`` returned, in its groups: the float32
        ``(T*B, C)`` gradient in the outputs, each sequence's rows times its entry of ``seq_scale`` (float32 ``(B,)`` on the
        device, or ``None``)."""
        B, T, P, y2d, a2d, group = st["B"], st["T"], self.n_pdf, st["y2d"], st["a2d"], st["group"]
        device = y2d.device
        with torch.cuda.device(device):
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            grad = torch.empty((T * B, P), dtype=torch.float32, device=device)
            ws = torch.empty(int(lib.tc_den_expected_accuracy_grad_workspace_bytes(self.ptr, group, T)), dtype=torch.uint8, device=device)
            for s0 in range(0, B, group):
                n = min(group, B - s0)
                yg, ag = _group_rows(y2d, s0, n, B, T), _group_rows(a2d, s0, n, B, T)
                gg = grad if n == B else torch.empty((T * n, P), dtype=torch.float32, device=device)
                check(lib.tc_den_expected_accuracy_dense_grad(
                    self.ptr, n, C.c_void_p(yg.data_ptr()), n * T, P, yg.stride(0),
                    None if st["fr"] is None else C.c_void_p(st["fr"][s0:s0 + n].data_ptr()), T, st["leaky"],
                    C.c_void_p(ag.data_ptr()), ag.stride(0), C.c_void_p(st["frame_acc"][s0:s0 + n].data_ptr()),
                    None if seq_scale is None else C.c_void_p(seq_scale[s0:s0 + n].data_ptr()), C.c_void_p(gg.data_ptr()), P,
                    C.c_void_p(ws.data_ptr()), ws.numel(), device.index, stream), "tc_den_expected_accuracy_dense_grad")
                if n != B:
                    grad.view(T, B, P)[:, s0:s0 + n].copy_(gg.view(T, n, P))
        return grad

    def sample_paths(self, nnet_output, num_samples, frames=None, leaky_hmm_coefficient=1e-5, generator=None, uniforms=None,
                     return_states=False, max_workspace_bytes=1 << 30, workspace=None, n_batch=None):
        """``num_samples`` paths a sequence drawn from this graph's path posterior under ``nnet_output``
        (``tc_den_sample_paths``): exact samples of ``P(path | y)`` of the denominator's own model -- outputs clamped to
        +-30, the graph's initial probabilities, every state final and the leaky-HMM transitions.  It is ``best_path`` with
        draws where that one maximises.  Returns ``pdfs``, int32 ``(B, K, Tmax)``, 0-based, or with ``return_states``
        ``(pdfs, states)``, ``states`` int32 ``(B, K, Tmax + 1, 2)``: the state a path entered level ``t`` in and the one it
        left it from, which differ where a leak happened.  ``-1`` in padding slots, and everywhere for a sequence with a NaN
        or an infinity in its valid frames or whose forward pass under- or overflows.

        The random numbers are an input: ``uniforms``, float32 ``(B, K, Tmax + 1, 3)`` in ``[0, 1)`` on the output's device
        (``include/torchain_hip.h`` says which decision each one takes), or ``None`` for
        ``torch.rand((B, K, Tmax + 1, 3), generator=generator, device=...)``.  A sample depends on its sequence's rows of
        ``nnet_output``, on its own uniforms, the graph and the coefficient alone.

        ``nnet_output``, ``frames`` and ``n_batch`` are ``best_path``'s: contiguous ``(B, C, T)`` float32 / bfloat16 / float16
        or 2-D float32 ``(T*B, C)`` (row ``t*B + b``); anything that is not 2-D float32 is copied into such a matrix first
        (``tc_rows_gather``).  Shapes, dtypes and lengths are checked here, before any library call.  The call keeps every
        state's forward probability of every frame, ``(Tmax + 1) * 4 * (states rounded up to 4)`` bytes a sequence; beyond
        ``max_workspace_bytes`` (or the size of ``workspace``, a CUDA uint8 tensor to reuse) consecutive groups of sequences
        run one after the other with the bits of one call.  Asynchronous on the current stream; no autograd:
        ``functions.sampled_risk_surrogate`` turns the samples and their risks into a gradient."""
        who = "sample_paths"
        x, B, T, lengths = self._accuracy_arguments(who, nnet_output, frames, n_batch)
        P, device = self.n_pdf, x.device
        if isinstance(num_samples, bool) or not isinstance(num_samples, (int, np.integer)) or int(num_samples) < 1:
            raise ValueError("%s: num_samples must be an int >= 1, got %r" % (who, num_samples))
        K = int(num_samples)
        leaky = float(leaky_hmm_coefficient)
        if not (0.0 <= leaky < float("inf")):
            raise ValueError("%s: the leaky-HMM coefficient must be finite and >= 0, got %r" % (who, leaky))
        if uniforms is not None:
            if generator is not None:
                raise ValueError("%s: give `uniforms` or `generator`, not both" % who)
            if not isinstance(uniforms, torch.Tensor) or uniforms.device != device or uniforms.dtype != torch.float32:
                raise ValueError("%s: uniforms must be a float32 tensor on the output's device (%s)" % (who, device))
            if tuple(uniforms.shape) != (B, K, T + 1, 3):
                raise ValueError("%s: uniforms of shape %s are not (%d, %d, %d, 3)" % (who, tuple(uniforms.shape), B, K, T + 1))
        elif generator is not None and not isinstance(generator, torch.Generator):
            raise TypeError("%s: generator must be a torch.Generator, got %s" % (who, type(generator).__name__))
        if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8
                                      or workspace.device != device or not workspace.is_contiguous()):
            raise ValueError("%s: workspace must be a contiguous uint8 tensor on the output's device" % who)
        need = lambda n: int(lib.tc_den_sample_paths_workspace_bytes(self.ptr, n, T))  # noqa: E731  (host arithmetic only)
        cap = int(max_workspace_bytes) if workspace is None else min(int(max_workspace_bytes), workspace.numel())
        group = B
        if need(B) > cap:
            if need(1) > cap:
                raise ValueError("%s: one sequence needs %d bytes of workspace, %d are allowed" % (who, need(1), cap))
            group = max(1, min(B, cap // need(1)))
            while need(group) > cap:
                group -= 1
            while group < B and need(group + 1) <= cap:  # (the sizes are rounded up: as many sequences as fit)
                group += 1
        fr = None if lengths is None else torch.from_numpy(np.ascontiguousarray(lengths, dtype=np.int32)).to(device)
        with torch.cuda.device(device):
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            u = uniforms.detach().contiguous() if uniforms is not None else torch.rand((B, K, T + 1, 3), generator=generator,
                                                                                       device=device)
            y2d = self._accuracy_rows(x, B, T, stream)
            pdfs = torch.empty((B, K, T), dtype=torch.int32, device=device)
            states = torch.empty((B, K, T + 1, 2), dtype=torch.int32, device=device) if return_states else None
            ws = workspace if workspace is not None else torch.empty(need(group), dtype=torch.uint8, device=device)
            for s0 in range(0, B, group):
                n = min(group, B - s0)
                yg = _group_rows(y2d, s0, n, B, T)
                check(lib.tc_den_sample_paths(self.ptr, n, C.c_void_p(yg.data_ptr()), n * T, P, yg.stride(0),
                                              None if fr is None else C.c_void_p(fr[s0:s0 + n].data_ptr()), T, leaky, K,
                                              C.c_void_p(u[s0:s0 + n].data_ptr()), C.c_void_p(pdfs[s0:s0 + n].data_ptr()),
                                              None if states is None else C.c_void_p(states[s0:s0 + n].data_ptr()),
                                              C.c_void_p(ws.data_ptr()), ws.numel(), device.index, stream),
                      "tc_den_sample_paths")
        return (pdfs, states) if return_states else pdfs


def _group_rows(m, s0, n, B, T):
    """Sequences ``s0 .. s0 + n - 1`` of a frame-major matrix ``(T*B, C)`` with unit column stride as a matrix ``(T*n, C)`` of
    their own, row ``t*n + s``: the matrix itself for the whole batch, a view for one sequence, a copy otherwise."""
    if n == B:
        return m
    rs, cols = m.stride(0), m.shape[1]
    g = torch.as_strided(m, (T, n, cols), (B * rs, rs, 1), m.storage_offset() + s0 * rs)
    return g[:, 0] if n == 1 else g.reshape(T * n, cols)


class Supervision:
    """Reference ``io.py:20-31``: wraps a supervision handle and exposes ``n_pdf``, ``n_batch``,
    ``n_frame``, ``shape``.  A null handle raises ``ValueError`` exactly like the reference (its
    iterators skip such batches, ``io.py:105-110``)."""

    def __init__(self, ptr):
        self.ptr = ptr if isinstance(ptr, C.c_void_p) else C.c_void_p(ptr)
        if not self.ptr:
            raise ValueError("null supervision ptr")
        self.n_pdf = lib.tc_supervision_num_pdf(self.ptr)
        self.n_batch = lib.tc_supervision_num_sequence(self.ptr)
        self.n_frame = lib.tc_supervision_num_frame(self.ptr)
        self.shape = (self.n_batch, self.n_frame, self.n_pdf)

    @classmethod
    def from_fst(cls, weight, num_sequences, frames_per_sequence, label_dim, arc_begin, ilabel, arc_weight,
                 nextstate, final):
        """Builds the handle from the five fields of [K] chain::Supervision the path uses
        (``src/my_lib_example.cpp:82-95``); the FST is the merged acceptor in CSR form."""
        ab, il, nx = _i32(arc_begin), _i32(ilabel), _i32(nextstate)
        aw, fin = _f32(arc_weight), _f32(final)
        handle = C.c_void_p()
        check(lib.tc_supervision_create(C.byref(handle), float(weight), int(num_sequences), int(frames_per_sequence),
                                        int(label_dim), len(fin), _p(ab), _p(il), _p(aw), _p(nx), _p(fin)),
              "tc_supervision_create")
        return cls(handle)

    @classmethod
    def from_e2e_fsts(cls, weight, frames_per_sequence, label_dim, fsts, den_graph=None, normalization_scale=1.0,
                      any_size=False):
        """End-to-end supervision ([K] ``Supervision::e2e_fsts``): one acceptor per sequence, not unfolded in time.
        ``fsts`` is a list of per-sequence ``(start, arc_begin, ilabel, arc_weight, nextstate, final)`` in CSR form
        (``ilabel`` = pdf_id + 1, tropical costs, ``final`` = inf for a state that is not final).

        ``frames_per_sequence``: an int, or one length per sequence (a "ragged" minibatch of whole utterances).  Then
        ``n_frame`` and ``shape`` use the longest length ``Tmax``: every tensor keeps its ``(B, C, Tmax)`` / ``(Tmax * B, C)``
        shape, frames ``t >= frames[s]`` of sequence ``s`` are padding that influences nothing, and every gradient is
        exactly zero there.  The lengths live in the handle: ``chain_loss`` and the other calls take no new argument.

        ``den_graph``: a ``DenominatorGraph`` whose weights the FSTs do not carry yet -- they are composed with its
        normalization acceptor first (``DenominatorGraph.normalize_fsts``, costs times ``normalization_scale``: [K] e2e
        ``normalization_fst_scale``), which bounds the objective by 0.  A sequence without a path in the graph raises
        ``ValueError`` naming the sequences.  ``None``: the FSTs are taken as they are.

        ``any_size``: ``False`` refuses (``TC_ERR_UNSUPPORTED``) a sequence beyond 2048 states, 8192 arcs or 1024 distinct
        pdfs, what the kernel that keeps a whole sequence on chip holds.  ``True`` (``tc_supervision_create_e2e_any``) takes
        every sequence with ``16 * ceil4(states) + 4 * ceil4(distinct pdfs) + 2048 <= 163840`` -- about 8192 states with 4096
        distinct pdfs -- and any number of arcs: a batch with a sequence beyond the old limits takes a second kernel
        (``e2e_stats()``), one within them is the handle ``False`` makes, bit for bit.  Acceptors composed with a
        ``den_graph`` and long transcripts are what needs it.  It is a keyword, not the default, only because a test pins the
        refusal of the default call; nothing else depends on it."""
        fsts = list(fsts)
        if not fsts:
            raise ValueError("from_e2e_fsts: no FSTs")
        if den_graph is not None:
            fsts = _normalized("from_e2e_fsts", den_graph, fsts, True, normalization_scale, label_dim)
        ragged = not np.isscalar(frames_per_sequence) and np.ndim(frames_per_sequence) > 0
        if ragged:
            lengths = np.asarray(frames_per_sequence)
            if lengths.shape != (len(fsts),) or lengths.dtype.kind not in "iu":
                raise ValueError("from_e2e_fsts: frames_per_sequence must be an int or one int per sequence")
            lengths = _i32(lengths)
        seq_begin, starts, ab, il, aw, nx, fin = [0], [], [np.zeros(1, np.int32)], [], [], [], []
        arcs = 0
        for start, arc_begin, ilabel, arc_weight, nextstate, final in fsts:
            arc_begin = np.asarray(arc_begin, dtype=np.int64)
            final = np.asarray(final, dtype=np.float32).ravel()
            if arc_begin.shape != (len(final) + 1,) or arc_begin[0] != 0:
                raise ValueError("from_e2e_fsts: arc_begin must have len(final) + 1 entries starting at 0")
            if any(np.asarray(x).size != arc_begin[-1] for x in (ilabel, arc_weight, nextstate)):
                raise ValueError("from_e2e_fsts: sequence %d: ilabel, arc_weight and nextstate must have arc_begin[-1] "
                                 "entries" % len(starts))
            seq_begin.append(seq_begin[-1] + len(final))
            starts.append(int(start))
            ab.append((arc_begin[1:] + arcs).astype(np.int32))
            arcs += int(arc_begin[-1])
            il.append(np.asarray(ilabel, dtype=np.int32).ravel())
            aw.append(np.asarray(arc_weight, dtype=np.float32).ravel())
            nx.append(np.asarray(nextstate, dtype=np.int32).ravel())
            fin.append(final)
        sb, st = _i32(seq_begin), _i32(starts)
        ab, il, nx = _i32(np.concatenate(ab)), _i32(np.concatenate(il)), _i32(np.concatenate(nx))
        aw, fin = _f32(np.concatenate(aw)), _f32(np.concatenate(fin))
        handle = C.c_void_p()
        if any_size:
            check(lib.tc_supervision_create_e2e_any(C.byref(handle), float(weight), len(fsts), 0 if ragged else int(frames_per_sequence),
                                                    _p(lengths) if ragged else None, int(label_dim), _p(sb), _p(st), _p(ab),
                                                    _p(il), _p(aw), _p(nx), _p(fin)), "tc_supervision_create_e2e_any")
            return cls(handle)
        if ragged:
            check(lib.tc_supervision_create_e2e_ragged(C.byref(handle), float(weight), len(fsts), _p(lengths), int(label_dim),
                                                       _p(sb), _p(st), _p(ab), _p(il), _p(aw), _p(nx), _p(fin)),
                  "tc_supervision_create_e2e_ragged")
            return cls(handle)
        check(lib.tc_supervision_create_e2e(C.byref(handle), float(weight), len(fsts), int(frames_per_sequence),
                                            int(label_dim), _p(sb), _p(st), _p(ab), _p(il), _p(aw), _p(nx), _p(fin)),
              "tc_supervision_create_e2e")
        return cls(handle)

    @classmethod
    def from_fsts(cls, weight, frames_per_sequence, label_dim, fsts, den_graph=None, normalization_scale=1.0):
        """Regular supervisions of unequal lengths (a "ragged" minibatch of whole utterances): one time-unfolded acceptor
        per sequence, as alignments and lattices give them.  ``fsts`` is a list of per-sequence
        ``(arc_begin, ilabel, arc_weight, nextstate, final)`` in CSR form -- each what ``from_fst`` takes with
        ``num_sequences = 1``: state 0 the start, states in time order, every path exactly that sequence's number of arcs
        long, ``ilabel`` = pdf_id + 1, tropical costs, ``final`` = inf for a state that is not final.
        ``frames_per_sequence``: one int per sequence.

        ``n_frame`` and ``shape`` use the longest length ``Tmax``, as for ``from_e2e_fsts`` with a list of lengths: every
        tensor keeps its ``(B, C, Tmax)`` / ``(Tmax * B, C)`` shape, frames ``t >= frames[s]`` of sequence ``s`` are padding
        that influences nothing, and every gradient is exactly zero there.  For every sequence the numerator computes the
        bits it computes on that sequence alone.

        ``den_graph``, ``normalization_scale``: as for ``from_e2e_fsts`` -- the FSTs are composed with the graph's
        normalization acceptor first, a sequence without a path in the graph raises ``ValueError`` naming the sequences."""
        fsts = list(fsts)
        if not fsts:
            raise ValueError("from_fsts: no FSTs")
        if den_graph is not None:
            fsts = _normalized("from_fsts", den_graph, fsts, False, normalization_scale, label_dim)
        lengths = np.asarray(frames_per_sequence)
        if lengths.shape != (len(fsts),) or lengths.dtype.kind not in "iu":
            raise ValueError("from_fsts: frames_per_sequence must be one int per sequence")
        lengths = _i32(lengths)
        seq_begin, ab, il, aw, nx, fin = [0], [np.zeros(1, np.int32)], [], [], [], []
        arcs = 0
        for arc_begin, ilabel, arc_weight, nextstate, final in fsts:
            arc_begin = np.asarray(arc_begin, dtype=np.int64)
            final = np.asarray(final, dtype=np.float32).ravel()
            if arc_begin.shape != (len(final) + 1,) or arc_begin[0] != 0:
                raise ValueError("from_fsts: arc_begin must have len(final) + 1 entries starting at 0")
            if any(np.asarray(x).size != arc_begin[-1] for x in (ilabel, arc_weight, nextstate)):
                raise ValueError("from_fsts: sequence %d: ilabel, arc_weight and nextstate must have arc_begin[-1] "
                                 "entries" % (len(seq_begin) - 1))
            seq_begin.append(seq_begin[-1] + len(final))
            ab.append((arc_begin[1:] + arcs).astype(np.int32))
            arcs += int(arc_begin[-1])
            il.append(np.asarray(ilabel, dtype=np.int32).ravel())
            aw.append(np.asarray(arc_weight, dtype=np.float32).ravel())
            nx.append(np.asarray(nextstate, dtype=np.int32).ravel())
            fin.append(final)
        sb = _i32(seq_begin)
        ab, il, nx = _i32(np.concatenate(ab)), _i32(np.concatenate(il)), _i32(np.concatenate(nx))
        aw, fin = _f32(np.concatenate(aw)), _f32(np.concatenate(fin))
        handle = C.c_void_p()
        check(lib.tc_supervision_create_ragged(C.byref(handle), float(weight), len(fsts), _p(lengths), int(label_dim),
                                               _p(sb), _p(ab), _p(il), _p(aw), _p(nx), _p(fin)),
              "tc_supervision_create_ragged")
        return cls(handle)

    @classmethod
    def from_sequences(cls, sups, den_graph=None, normalization_scale=1.0):
        """A ragged minibatch from single-sequence regular supervisions (``torchain_amd.synth.SupFst`` with
        ``num_sequences == 1``: what the egs readers return for one eg), each of its own ``frames_per_sequence``.  They must
        share ``weight`` and ``label_dim``.  ``den_graph``, ``normalization_scale``: as for ``from_fsts``."""
        sups = list(sups)
        if not sups:
            raise ValueError("from_sequences: no supervisions")
        for i, s in enumerate(sups):
            if isinstance(s, _egs.E2eSup):
                raise ValueError("from_sequences: supervision %d is an end-to-end one (from_e2e_fsts takes their lengths)" % i)
            if int(s.num_sequences) != 1:
                raise ValueError("from_sequences: supervision %d has %d sequences, not 1" % (i, s.num_sequences))
            if float(s.weight) != float(sups[0].weight) or int(s.label_dim) != int(sups[0].label_dim):
                raise ValueError("from_sequences: supervision %d differs from the first in weight or label_dim" % i)
        return cls.from_fsts(sups[0].weight, [int(s.frames_per_sequence) for s in sups], sups[0].label_dim,
                             [(s.arc_begin, s.ilabel, s.arc_weight, s.nextstate, s.final) for s in sups],
                             den_graph=den_graph, normalization_scale=normalization_scale)

    @classmethod
    def from_alignments(cls, weight, pdfs, label_dim, frames=None, den_graph=None, normalization_scale=1.0):
        """Regular supervisions from frame-level pdf alignments, e.g. what ``best_path`` of a flat-start model's handle
        returns: one linear acceptor per sequence at cost 0, through ``from_fsts``.  ``pdfs``: int ``(B, Tmax)``, 0-based,
        ``-1`` in the padding; ``frames``: the sequences' lengths, by default the count of non-negative entries of each
        row.  With ``den_graph`` the alignment carries the graph's weights, ``-log pi - sum log w`` summed over the start
        states that admit it.  ``ValueError``: a ``-1`` inside a sequence (``best_path`` found no path for it), a pdf outside
        ``label_dim``, an alignment the graph does not contain.  Tolerance around the phone boundaries needs the tree and
        the transition model and stays with the caller, who passes the widened FSTs to ``from_fsts``."""
        if isinstance(pdfs, torch.Tensor):
            pdfs = pdfs.detach().cpu().numpy()
        pdfs = np.asarray(pdfs)
        if pdfs.ndim != 2 or pdfs.dtype.kind not in "iu" or pdfs.shape[0] < 1:
            raise ValueError("from_alignments: pdfs must be an int (B, Tmax) array")
        B, Tmax = pdfs.shape
        if frames is None:
            lengths = (pdfs >= 0).sum(axis=1)
        else:
            lengths = frames.detach().cpu().numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)
            if lengths.shape != (B,) or lengths.dtype.kind not in "iu":
                raise ValueError("from_alignments: frames must be one int per sequence")
        bad = [b for b in range(B) if not 1 <= int(lengths[b]) <= Tmax]
        if bad:
            raise ValueError("from_alignments: sequences %s have no frames (or more than the array holds)" % bad)
        bad = [b for b in range(B) if (pdfs[b, :int(lengths[b])] < 0).any() or (pdfs[b, int(lengths[b]):] != -1).any()]
        if bad:
            raise ValueError("from_alignments: sequences %s have a -1 inside their frames or a pdf in their padding" % bad)
        bad = [b for b in range(B) if (pdfs[b, :int(lengths[b])] >= int(label_dim)).any()]
        if bad:
            raise ValueError("from_alignments: sequences %s have a pdf outside 0 .. %d" % (bad, int(label_dim) - 1))
        fsts = []
        for b in range(B):
            n = int(lengths[b])
            final = np.full(n + 1, np.inf, np.float32)
            final[n] = 0.0
            fsts.append((np.minimum(np.arange(n + 2), n).astype(np.int32), (pdfs[b, :n] + 1).astype(np.int32),
                         np.zeros(n, np.float32), np.arange(1, n + 1, dtype=np.int32), final))
        return cls.from_fsts(weight, [int(x) for x in lengths], label_dim, fsts, den_graph=den_graph,
                             normalization_scale=normalization_scale)

    @property
    def is_e2e(self):
        """True for an end-to-end supervision (``from_e2e_fsts``)."""
        return bool(lib.tc_supervision_is_e2e(self.ptr))

    @property
    def is_ragged(self):
        """True for a supervision made with one length per sequence (``from_fsts``, ``from_sequences``, ``from_e2e_fsts``
        with a list of lengths), also when the lengths are all equal."""
        return bool(lib.tc_supervision_is_ragged(self.ptr))

    @property
    def frames(self):
        """The sequences' lengths (numpy int32, ``n_batch`` entries; all ``n_frame`` unless ``is_ragged``, regular and
        end-to-end supervisions alike)."""
        out = np.zeros(self.n_batch, dtype=np.int32)
        check(lib.tc_supervision_frames(self.ptr, _p(out)), "tc_supervision_frames")
        return out

    @classmethod
    def from_synth(cls, sup, any_size=False):
        """From a ``torchain_amd.synth.SupFst``, or an ``egs.E2eSup`` (what the egs readers return for ``<End2End>``
        egs; ``any_size``: as for ``from_e2e_fsts``, not read for a ``SupFst``)."""
        if isinstance(sup, _egs.E2eSup):
            return cls.from_e2e_fsts(sup.weight, sup.frames_per_sequence, sup.label_dim, sup.fsts, any_size=any_size)
        return cls.from_fst(sup.weight, sup.num_sequences, sup.frames_per_sequence, sup.label_dim, sup.arc_begin,
                            sup.ilabel, sup.arc_weight, sup.nextstate, sup.final)

    @property
    def weight(self):
        return lib.tc_supervision_weight(self.ptr)

    def stats(self):
        """What the numerator will do with this (regular) supervision, known on the host before anything runs
        (``tc_supervision_stats``): sizes of the largest sequence, of its widest time level, the LDS either numerator
        kernel would need, and ``kernel``: ``"resident"`` (a whole sequence on chip), ``"windowed"`` (two time levels
        on chip; sequences of any size) or ``"unsupported"`` (a single level beyond LDS: ``chain_loss`` will raise).
        ``route`` is the same as a number (0, 1, negative error code).  End-to-end supervisions raise."""
        out = np.zeros(12, np.int64)
        check(lib.tc_supervision_stats(self.ptr, _p(out)), "tc_supervision_stats")
        keys = ("sequences", "frames", "max_states", "max_arcs", "max_uniq", "max_level_states", "max_level_arcs",
                "max_frame_uniq", "resident_lds_bytes", "windowed_lds_bytes", "history_bytes", "route")
        d = dict(zip(keys, (int(x) for x in out)))
        d["kernel"] = {0: "resident", 1: "windowed"}.get(d["route"], "unsupported")
        return d

    def e2e_stats(self):
        """What the numerator will do with this end-to-end supervision, known on the host (``tc_supervision_e2e_stats``):
        the sizes of the largest sequence, the LDS either kernel would need, the kernel scratch in the handle's pool slot, and
        ``kernel``: ``"resident"`` (a whole sequence on chip, within 2048 states / 8192 arcs / 1024 distinct pdfs) or
        ``"large"`` (arc occupations in the pool slot; ``from_e2e_fsts(..., any_size=True)``).  ``route`` is the same as a
        number (0, 1).  Regular supervisions raise (``stats()`` is theirs)."""
        out = np.zeros(8, np.int64)
        check(lib.tc_supervision_e2e_stats(self.ptr, _p(out)), "tc_supervision_e2e_stats")
        keys = ("sequences", "max_states", "max_arcs", "max_pdfs", "resident_lds_bytes", "large_lds_bytes", "scratch_bytes",
                "route")
        d = dict(zip(keys, (int(x) for x in out)))
        d["kernel"] = {0: "resident", 1: "large"}[d["route"]]
        return d

    def best_path(self, nnet_output):
        """The single most likely path of every sequence under ``nnet_output``: the frame-level pdf alignment
        (``tc_supervision_best_path``), for regular and end-to-end handles, uniform and ragged.  Returns ``(pdfs, scores)``
        on the input's device: ``pdfs`` int32 ``(B, Tmax)``, the 0-based pdf of every frame and ``-1`` in a ragged handle's
        padding frames; ``scores`` float64 ``(B,)``, the path's log score (sum of ``y_t(pdf_t) - arc cost``, minus the final
        cost; the supervision's ``weight`` does not enter).  A sequence without a path of exactly its number of frames gets
        ``-inf`` and ``-1`` in all its frames.

        ``nnet_output`` is what ``chain_loss`` takes: ``(B, C, T)`` or ``(T*B, C)``.  2-D float32 with unit column stride and
        contiguous ``(B, C, T)`` in float32, bfloat16 or float16 are read where they lie; any other view or dtype goes through
        ``.contiguous()`` (and ``.float()``) first -- alignment is not a hot path.  No autograd: the input is detached, the
        outputs carry no graph.  Asynchronous on the current stream; the history in the handle's pool slot is scratch, so
        a ``chain_loss`` on the handle is not affected."""
        x = nnet_output.detach()
        if not x.is_cuda:
            raise ValueError("best_path: nnet_output must be a CUDA tensor (only the HIP implementation is available)")
        S, T, P = self.n_batch, self.n_frame, self.n_pdf
        want = (S, P, T) if x.dim() == 3 else (S * T, P)
        if x.dim() not in (2, 3) or tuple(x.shape) != want:
            raise ValueError("best_path: nnet output of shape %s does not match the supervision (%s expected)"
                             % (tuple(x.shape), want))
        dtypes = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}  # TC_DTYPE_*
        if x.dtype not in dtypes or (x.dim() == 2 and x.dtype != torch.float32):
            x = x.float()
        if x.dim() == 3 and not x.is_contiguous():
            x = x.contiguous()
        if x.dim() == 2 and (x.stride(1) != 1 or x.stride(0) < P):
            x = x.contiguous()
        device = x.device
        pdfs = torch.empty((S, T), dtype=torch.int32, device=device)
        scores = torch.empty((S,), dtype=torch.float64, device=device)
        with torch.cuda.device(device):
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            check(lib.tc_supervision_best_path(self.ptr, C.c_void_p(x.data_ptr()), dtypes[x.dtype], int(x.dim() == 3), S * T, P,
                                               x.stride(0) if x.dim() == 2 else 0, C.c_void_p(pdfs.data_ptr()),
                                               C.c_void_p(scores.data_ptr()), device.index, stream),
                  "tc_supervision_best_path")
        return pdfs, scores

    def posteriors(self, nnet_output, pdf_class=None):
        """The numerator's occupation posteriors ``gamma_num_t(j)`` under ``nnet_output``, dense float32 ``(T*B, C)`` (row
        ``t*B + b``) on the input's device: what Kaldi's chain-sMBR scores the denominator's paths against
        (``DenominatorGraph.expected_accuracy_dense``, ``functions.den_expected_accuracy_dense``).  Regular and end-to-end
        handles, uniform and ragged, on whichever numerator kernel the handle takes: ``tc_num_forward_backward`` into a zeroed
        matrix, divided by the handle's weight (a weight of 0 raises ``ValueError``).  The rows of a sequence's valid frames sum
        to 1; padding rows, and every row of a sequence without a path of its length, are +0.

        ``pdf_class``: ``None``, or ``n_pdf`` ints that pool the posteriors by class, ``a_t(j) = sum of gamma_num_t(k) over the
        k with class(k) == class(j)`` -- an MPFE-style accuracy (a pdf -> phone map); rows then sum to the sizes of the
        classes met.  ``nnet_output`` is what ``chain_loss`` takes: 2-D float32 ``(T*B, C)``, or ``(B, C, T)`` in float32 /
        bfloat16 / float16 (copied into such a matrix first).  No autograd: the result is a constant, as in Kaldi.  The handle's
        pool slot is scratch here as for ``best_path``: a training step on the handle gives the same bits before and after."""
        x = nnet_output.detach() if isinstance(nnet_output, torch.Tensor) else nnet_output
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError("posteriors: nnet_output must be a CUDA tensor (only the HIP implementation is available)")
        S, T, P = self.n_batch, self.n_frame, self.n_pdf
        want = (S, P, T) if x.dim() == 3 else (S * T, P)
        if x.dim() not in (2, 3) or tuple(x.shape) != want:
            raise ValueError("posteriors: nnet output of shape %s does not match the supervision (%s expected)"
                             % (tuple(x.shape), want))
        dtypes = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}  # TC_DTYPE_*
        if x.dtype not in dtypes or (x.dim() == 2 and x.dtype != torch.float32):
            raise TypeError("posteriors: the output must be float32 (or, as (B, C, T), bfloat16 or float16), got %s" % x.dtype)
        weight = float(self.weight)
        if not (weight != 0.0 and abs(weight) < float("inf")):
            raise ValueError("posteriors: the supervision's weight is %r; the posteriors are the derivative divided by it" % weight)
        device = x.device
        cls = None
        if pdf_class is not None:
            cls = pdf_class.detach() if isinstance(pdf_class, torch.Tensor) else torch.from_numpy(np.asarray(pdf_class))
            if cls.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8) or tuple(cls.shape) != (P,):
                raise ValueError("posteriors: pdf_class must be an int tensor or array of shape (%d,)" % P)
            cls = cls.to(device=device, dtype=torch.int64)
        with torch.cuda.device(device):
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            if x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= P and x.data_ptr() % 4 == 0:
                y2d = x
            else:  # (b, t, :) rows of a channel-last tensor of `dtype` -> float32 row t*B + b
                rows = x.transpose(1, 2).contiguous() if x.dim() == 3 else x.reshape(T, S, P).transpose(0, 1).contiguous()
                y2d = torch.empty((T * S, P), dtype=torch.float32, device=device)
                check(lib.tc_rows_gather(C.c_void_p(rows.data_ptr()), dtypes[x.dtype], S, P, T, T * P, P,
                                         C.c_void_p(y2d.data_ptr()), P, device.index, stream), "tc_rows_gather")
            post = torch.zeros((T * S, P), dtype=torch.float32, device=device)
            ws = torch.empty(256 * ((S * 8 + 255) // 256) + 256, dtype=torch.uint8, device=device)  # a log-prob per sequence
            check(lib.tc_num_forward_backward(self.ptr, C.c_void_p(y2d.data_ptr()), S * T, P, y2d.stride(0),
                                              C.c_void_p(post.data_ptr()), P, None, C.c_void_p(ws.data_ptr()), ws.numel(),
                                              device.index, stream), "tc_num_forward_backward")
            post /= weight
            # a sequence without a path: its log-prob is not finite, whatever the kernel left in its rows
            alive = torch.isfinite(ws[:S * 8].view(torch.float64))
            post = torch.where(alive.view(1, S, 1), post.view(T, S, P), post.new_zeros(())).view(T * S, P)
            if cls is not None:  # pooled by class, in double: exact for posteriors and the same in every call
                inv = torch.unique(cls, return_inverse=True)[1]
                member = torch.zeros((P, int(inv.max()) + 1), dtype=torch.float64, device=device)
                member[torch.arange(P, device=device), inv] = 1.0
                post = (post.double() @ member)[:, inv].float().contiguous()
        return post

    def __del__(self, _free=lib.tc_supervision_free):
        ptr = getattr(self, "ptr", None)
        if ptr:
            _free(ptr)
            self.ptr = None


# ---- Kaldi chain-egs readers (reference io.py:60-175) ------------------------------------------------------
class Example:
    """``Example(rspec)``: sequential reader of chain egs (reference ``io.py:60-113`` over Kaldi's
    SequentialNnetChainExampleReader, ``src/my_lib_example.cpp:35-127``).  ``rspec`` is a Kaldi rspecifier
    (``ark:file``, ``ark,bg:file``, ``scp:file``, ``ark:command |``).  Same surface as the reference: ``next()``,
    ``load_feats``, ``supervision``, ``indexes``, ``inputs``, ``value()``, iteration yielding
    ``((inp (B, F, T_in), aux), Supervision)``.

    One deliberate difference: the reference's ``next()`` advances a reader that already stands on the first
    example, so its iteration silently drops the first example of every archive (and ends on a null supervision);
    here every example is delivered.  ``deriv_weights`` -- which the reference drops (``README.md:41``) -- is
    available as a property."""

    def __init__(self, rspec):
        self.rspec = rspec
        self._it = _egs.iter_rspecifier(rspec)
        self._cur = None

    def next(self):
        try:
            _key, eg = next(self._it)
        except StopIteration:
            self._cur = None
            return False
        self._cur = eg
        return True

    def _need(self):
        if self._cur is None:
            raise ValueError("null supervision ptr")  # what the reference raises past the end (io.py:23-24)
        return self._cur

    def load_feats(self, inp=None, aux=None):
        """Reference ``my_lib_example_feats``: number of inputs of the current example (tensors are returned by
        ``inputs``; the in-place TH resize of the reference has no counterpart)."""
        return len(self._need()["inputs"])

    @property
    def supervision(self):
        cur = self._need()
        if "_handle" not in cur:  # (RandExample's look-ahead has usually built it already)
            cur["_handle"] = Supervision.from_synth(cur["outputs"][0]["supervision"])
        return cur["_handle"]

    @property
    def indexes(self):
        """(B, T) LongTensor of the output frames' ``t`` (reference ``my_lib_example_reader_indexes``)."""
        out = self._need()["outputs"][0]
        sup = out["supervision"]
        t = out["indexes"][:, 1].reshape(sup.frames_per_sequence, sup.num_sequences)
        return torch.from_numpy(np.ascontiguousarray(t.T).astype(np.int64))

    @property
    def deriv_weights(self):
        """(T*B,) float tensor, frame-major like the nnet output rows ([K] NnetChainSupervision::deriv_weights)."""
        return torch.from_numpy(self._need()["outputs"][0]["deriv_weights"].astype(np.float32))

    @property
    def inputs(self):
        ins = self._need()["inputs"]
        if len(ins) == 1:
            return torch.from_numpy(ins[0]["features"]), None
        if len(ins) == 2:
            return torch.from_numpy(ins[0]["features"]), torch.from_numpy(ins[1]["features"])
        raise ValueError("unsupported number of inputs (up to 2): %d" % len(ins))

    def value(self):
        supervision = self.supervision
        n_batch, n_out_frame, n_pdf = supervision.shape
        inp, aux = self.inputs
        if inp is not None:
            inp = inp.view(n_batch, -1, inp.shape[1]).transpose(1, 2)
        return (inp, aux), supervision

    def __iter__(self):
        while self.next():
            try:
                yield self.value()
            except ValueError:
                continue


def feats(egs):
    """Reference ``io.py:34-48`` (broken there: it refers to ``self``): (input, aux-or-None) of the current example."""
    if isinstance(egs, Example):
        return egs.inputs
    raise ValueError("unknown reader type")


@contextmanager
def open_example(cmd):
    """Reference ``io.py:116-131``: runs ``cmd`` (e.g. ``nnet3-chain-copy-egs ... ark:-``) and reads the egs it writes
    to stdout.  The reference goes through a FIFO and Kaldi's ``ark,bg:`` reader; a pipe does the same job."""
    set_kaldi_device()
    example = Example("ark:" + cmd + " |")
    try:
        yield example
    finally:
        del example


def print_key_length(scp_path, len_file="/dev/stdout"):
    """Reference ``io.py:134-135`` / ``my_lib_example_rand.cpp:168-177``: ``key frames_per_sequence`` per example."""
    with open(len_file, "w") as f:
        for key, eg in _egs.iter_rspecifier(scp_path):
            f.write("%s %d\n" % (key, eg["outputs"][0]["supervision"].frames_per_sequence))


class RandExample(Example):
    """``RandExample(scp_path, seed, batchsize, len_file="")``: random-access reader that groups examples of equal
    ``frames_per_sequence`` into minibatches, shuffles inside and across groups and merges each minibatch
    ([K] MergeChainExamples) -- reference ``io.py:138-175`` over ``src/my_lib_example_rand.cpp:35-177``.  The
    length file (``scp_path + ".len"`` unless given) holds ``key length`` pairs; without it the lengths are read
    from the egs.  The shuffle of the default (native) reader is a Fisher-Yates pass over ``std::mt19937`` draws
    (``csrc/rand_reader.cpp``): the reference's generator, but not the draw order of its ``std::shuffle``, whose algorithm
    is not specified -- and not the order round 3's Python reader (``native=False``: NumPy's MT19937 shuffle) gives for
    the same ``seed``: the batch order for a given seed changed when the native reader became the default in round 4."""

    def __init__(self, scp_path, seed, batchsize, len_file="", prefetch=True, rank=0, world=1, native=True, device=None,
                 order="sorted"):
        """``rank`` / ``world``: this process's share of a data-parallel job (every rank forms the same shuffled list of
        minibatches from ``seed`` and takes every ``world``-th; all ranks get the same number).  ``native`` (default): the
        whole reader -- bucketing, shuffle, look-ahead threads, merge, supervision handles -- is the library's
        ``tc_rand_reader_*`` handle, as the reference's is ``my_lib_example_rand_reader_*`` (``src/my_lib.h:8-17``);
        ``device`` is the GPU the batches are for: given explicitly, the look-ahead threads also fill the pinned staging of
        each supervision's upload (they then touch that GPU: ``hipSetDevice`` / pinned allocations on worker threads); left
        ``None``, building the reader touches no GPU -- a script may still fork or re-launch itself -- and the staging starts
        with the first ``next()`` made after the process has initialised CUDA, for the then current device.
        ``native=False`` keeps the Python statement of it below (NumPy's MT19937 shuffle, a thread pool), which needs
        ``rank == 0, world == 1``.
        ``order``: ``"sorted"`` (default; lengths ascending, a Fisher-Yates pass that is the same on every platform) or
        ``"reference"``: the reference's ``shuffle_keys`` restated on the same standard-library calls
        (``src/my_lib_example_rand.cpp:119-141``: ``std::unordered_map`` iteration, ``std::shuffle`` over ``std::mt19937``) --
        the batch lists a reference built against libstdc++ forms for the same ``seed``, epoch for epoch (native reader
        only; ``rank`` / ``world`` sharding applies on top)."""
        assert os.path.exists(scp_path)
        self.scp_path = scp_path
        self.rspec = scp_path
        self.batchsize = int(batchsize)
        self._native = None
        if native:
            handle = C.c_void_p()
            # (True = 3 look-ahead threads: a batch of 64 x 150 frames costs one of them ~1.5 ms, a step 0.7 ms; with more
            # the training thread's own enqueue slows down -- 0.11 ms beside two readers, 0.39 beside four, 0.47 beside
            # eight on the test box -- and the step with it: profiles/r04_egs_steps.txt)
            depth = (3 if prefetch is True else int(prefetch)) if prefetch else 0
            if order not in ("sorted", "reference"):
                raise ValueError("order must be 'sorted' or 'reference'")
            rc = lib.tc_rand_reader_new_ordered(os.fsencode(scp_path), int(seed), int(batchsize), os.fsencode(len_file or ""),
                                                int(rank), int(world), depth, 1 if order == "reference" else 0, C.byref(handle))
            if rc != 0:
                raise _egs.EgsFormatError((lib.tc_rand_reader_last_error() or b"").decode() or "tc_rand_reader_new: %d" % rc)
            self._native = handle
            self._cur = None
            self._have = False
            # the GPU the minibatches are for: the look-ahead threads then also fill the pinned staging of each supervision's
            # upload, which otherwise falls to the training thread's first use of it.  Only an EXPLICIT device is set here:
            # asking torch for the current one would initialise the GPU context in a constructor (see the docstring).
            self._staging_device = None
            if device is not None:
                self._set_staging_device(int(torch.device("cuda", device).index if not isinstance(device, int) else device))
            return
        if rank != 0 or world != 1 or order != "sorted":
            raise ValueError("the Python reader does not shard and has one order: use native=True")
        # The next minibatches are prepared on background threads while the current one is in use (reading, parsing,
        # merging and building the supervision handle are library calls that release the interpreter lock): the
        # training thread finds its batch ready instead of re-opening and re-parsing every scp entry synchronously.
        # One batch costs about 1.6 ms of such work for 64 x 150 frames, a training-side step 0.7 ms: ``prefetch``
        # batches (True = 8) are kept under way, each on its own thread.
        self._depth = (8 if prefetch is True else int(prefetch)) if prefetch else 0
        self._pool = ThreadPoolExecutor(max_workers=self._depth) if self._depth else None
        self._pending = {}  # position -> future
        self._rng = np.random.RandomState(int(seed))
        self._where = {key: (p, off) for key, p, off in _egs.read_scp(scp_path)}
        self._length_to_keys = {}
        lf = len_file or scp_path + ".len"
        if os.path.exists(lf):
            toks = open(lf).read().split()
            for key, length in zip(toks[0::2], toks[1::2]):
                self._length_to_keys.setdefault(int(length), []).append(key)
        else:
            for key, (p, off) in self._where.items():
                eg = _egs.read_scp_entry(p, off)
                self._length_to_keys.setdefault(eg["outputs"][0]["supervision"].frames_per_sequence, []).append(key)
        self._n_data = sum(len(v) for v in self._length_to_keys.values())
        self._shuffle_keys()
        self._pos = -1
        self._cur = None

    def _set_staging_device(self, index):
        check(lib.tc_rand_reader_set_device(self._native, int(index)), "tc_rand_reader_set_device")
        self._staging_device = int(index)

    def _shuffle_keys(self):
        self._key_batch = []
        for length in sorted(self._length_to_keys):
            keys = list(self._length_to_keys[length])
            self._rng.shuffle(keys)
            for i in range(0, len(keys), self.batchsize):
                self._key_batch.append(keys[i:i + self.batchsize])
        self._rng.shuffle(self._key_batch)

    def reset(self):
        if self._native is not None:
            check(lib.tc_rand_reader_reset(self._native), "tc_rand_reader_reset")
            self._cur, self._have = None, False
            return
        self._drop_pending()
        self._pos = -1
        self._cur = None
        self._shuffle_keys()

    def _drop_pending(self):
        for fut in self._pending.values():
            fut.cancel()
        for fut in self._pending.values():
            try:
                fut.result()
            except Exception:  # (a cancelled or failed look-ahead is simply not used)
                pass
        self._pending = {}

    def _load(self, pos):
        # read + parse + merge in the library (tc_example_read), as the reference does in Kaldi, and the supervision
        # handle (tc_supervision_create: per-sequence split, time levels; 1.2 ms of host work for 64 x 150 frames) with
        # it: on the look-ahead thread both run beside the training step, outside the interpreter lock
        merged = _egs.read_merged_native([self._where[k] for k in self._key_batch[pos]])
        try:
            merged["_handle"] = Supervision.from_synth(merged["outputs"][0]["supervision"])
        except Exception:  # (reported when the batch is used: Example.supervision builds it again and raises there)
            pass
        return merged

    def __del__(self, _free=lib.tc_rand_reader_free):
        pool = getattr(self, "_pool", None)
        if pool is not None:
            pool.shutdown(wait=False)
        handle = getattr(self, "_native", None)
        if handle:
            _free(handle)
            self._native = None

    @property
    def n_batch(self):
        if self._native is not None:
            return lib.tc_rand_reader_num_batch(self._native)
        return len(self._key_batch)

    @property
    def n_data(self):
        if self._native is not None:
            return lib.tc_rand_reader_num_data(self._native)
        return self._n_data

    def batch_keys(self, batch):
        """The keys of this rank's minibatch ``batch`` of the current epoch (native reader)."""
        buf = C.create_string_buffer(1 << 16)
        n = lib.tc_rand_reader_batch_keys(self._native, int(batch), buf, len(buf))
        check(min(n, 0), "tc_rand_reader_batch_keys")
        return buf.value.decode().split()

    def _need(self):
        if self._native is not None and self._cur is None and self._have:
            # the minibatch the library holds, as the dict the numpy reader returns; the supervision handle the
            # look-ahead thread built comes with it
            sup = C.c_void_p()
            check(lib.tc_rand_reader_supervision_new(self._native, C.byref(sup)), "tc_rand_reader_supervision_new")
            handle = Supervision(sup)
            eg = C.c_void_p()
            check(lib.tc_rand_reader_take_example(self._native, C.byref(eg)), "tc_rand_reader_take_example")
            self._cur = _egs._wrap_native(eg)
            self._cur["_handle"] = handle
        return super()._need()

    def next(self):
        if self._native is not None:
            # (is_initialized() first: on ROCm is_available() itself initialises the runtime, and a reader built with
            # device=None promises to touch no GPU until the process has)
            if self._staging_device is None and torch.cuda.is_initialized():
                self._set_staging_device(torch.cuda.current_device())  # (the process uses the GPU by now: no new context)
            rc = lib.tc_rand_reader_next(self._native)
            self._cur = None
            self._have = rc == 1
            if rc < 0:
                raise _egs.EgsFormatError((lib.tc_rand_reader_last_error() or b"").decode() or "tc_rand_reader_next: %d" % rc)
            return rc == 1
        self._pos += 1
        if self._pos >= len(self._key_batch):
            self._cur = None
            return False
        fut = self._pending.pop(self._pos, None)
        self._cur = fut.result() if fut is not None else self._load(self._pos)
        if self._pool is not None:
            for pos in range(self._pos + 1, min(self._pos + 1 + self._depth, len(self._key_batch))):
                if pos not in self._pending:
                    self._pending[pos] = self._pool.submit(self._load, pos)
        return True
