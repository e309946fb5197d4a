"""ms per call of eval forward + explain.input_gradients of the full multimodal model, next to the training step's
forward + backward at the same batch (events on the current stream).
Usage: python tools/explain_bench.py [--batch 64] [--reps 10]"""
import argparse, os, sys
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--reps", type=int, default=10)
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ecgmm import explain
from ecgmm.config import Config
from ecgmm.hip import functional as HF
from ecgmm.multimodal_paper_modal_balance import ECGMultimodalModel
from oracle import fill

dev = torch.device("cuda:0")
img, sig, clin, lab = (t.to(dev) for t in fill.synthetic_batch(a.batch, clin_dim=24, salt=3))


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.reps


for cd in ("fp32", "bf16"):
    net = ECGMultimodalModel(type("Cfg", (Config,), {"compute_dtype": cd})).to(dev)

    def train_fwd_bwd():
        net.train()
        for p in net.parameters():
            p.grad = None
        out = net(img, sig, clin)
        HF.cross_entropy_plus(out[3], lab, out[4], 0.1).backward()

    def explain_call():
        explain.input_gradients(net, img, sig, clin)

    def cam_call():
        explain.grad_cam(net, img, sig, clin)

    print(f"B={a.batch} {cd}: training forward + backward {timed(train_fwd_bwd):.2f} ms, eval forward + input_gradients "
          f"{timed(explain_call):.2f} ms, eval forward + grad_cam {timed(cam_call):.2f} ms")
