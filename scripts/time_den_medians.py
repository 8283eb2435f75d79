"""Times tc_den_forward_backward (with derivative) of a workload for A/B runs of two libraries in turn (development aid):
60 warm-up launches, then median / min / max of 7 groups of 20 launches by CUDA events, and the log-prob, the status and a
SHA-1 of the derivative matrix on seeded outputs, so that two builds can be told apart or held equal.
  python scripts/time_den_medians.py [config] [S]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from torchain_amd import io, synth  # noqa: E402
from torchain_amd._lib import check, lib  # noqa: E402

cfgname = sys.argv[1] if len(sys.argv) > 1 else "C3"
cfg = synth.CONFIGS[cfgname]
S, T, P = cfg["S"], cfg["T"], cfg["P"]
if len(sys.argv) > 2:
    S = int(sys.argv[2])
fst = synth.config_den_fst(cfgname)
dev = torch.device("cuda", 0)
graph = io.DenominatorGraph(fst, P).prepare(dev)
torch.manual_seed(0)
y = torch.randn(S * T, P, device=dev)
lp = torch.zeros(1, dtype=torch.float64, device=dev)
stt = torch.full((1,), -1, dtype=torch.int32, device=dev)
deriv = torch.empty_like(y)
nbytes = lib.tc_chain_workspace_bytes(graph.ptr, S, T)
ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
stream = torch.cuda.current_stream()


def run():
    check(lib.tc_den_forward_backward(
        graph.ptr, S, C.c_void_p(y.data_ptr()), S * T, P, y.stride(0), cfg["leaky"], -1.0, cfg.get("l2", 0.0), 0,
        C.c_void_p(deriv.data_ptr()), deriv.stride(0), C.c_void_p(lp.data_ptr()), C.c_void_p(stt.data_ptr()),
        C.c_void_p(ws.data_ptr()), nbytes, 0, C.c_void_p(stream.cuda_stream)), "den")


for _ in range(60):
    run()
torch.cuda.synchronize()
res = []
for _ in range(7):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        run()
    e1.record()
    e1.synchronize()
    res.append(e0.elapsed_time(e1) / 20)
res.sort()
print("%s S=%d: median %.4f min %.4f max %.4f ms" % (cfgname, S, res[len(res) // 2], res[0], res[-1]))
import hashlib  # noqa: E402

print("   lp %.17g status %d deriv sha %s" % (float(lp), int(stt), hashlib.sha1(deriv.cpu().numpy().tobytes()).hexdigest()[:16]))
