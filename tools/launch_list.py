"""Launch list of one eager FOCAL step on MOD at batch 256 (bf16), via the library's launch trace.
usage: launch_list.py ROOT APE(0|1) OUT.json      ROOT: the tree whose focal_amd is imported (this one, or a checkout of another
commit built beside it); tools/launch_list_diff.py A.json B.json compares two lists as multisets of (kernel, grid, block)."""
import argparse, copy, json, os, sys
root, ape, out = os.path.abspath(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
for p in (root, os.path.join(root, "focal_amd", "src")):
    sys.path.insert(0, p)
import ctypes as C
import torch
from focal_amd import _lib
from models.FOCALModules import FOCAL
from models.loss import FOCALLoss
from models.SW_Transformer import SW_Transformer
from oracle.config import load_config
from oracle.weights import fill_state_dict_, synthetic_freq_input
from train_utils.optimizer import define_optimizer

cfg = copy.deepcopy(load_config())
cfg["SW_Transformer"]["APE"] = bool(ape)
args = argparse.Namespace(model="SW_Transformer", dataset="MOD", device=torch.device("cuda:0"), train_mode="contrastive",
                          learn_framework="FOCAL", stage="pretrain", task="vehicle_classification", tag=None,
                          dataset_config=cfg, compute_dtype="bf16")
net = SW_Transformer(args)
fill_state_dict_(net.state_dict())
net = net.to(args.device).train()
focal, loss_fn = FOCAL(args, net), FOCALLoss(args)
opt = define_optimizer(args, focal.parameters())
B = 256
dev = lambda d: {l: {m: v.to(args.device) for m, v in mm.items()} for l, mm in d.items()}
x1, x2 = dev(synthetic_freq_input(cfg, B, 101)), dev(synthetic_freq_input(cfg, B, 202))

def step():
    opt.zero_grad()
    f1, f2 = focal(x1, x2, proj_head=True)
    loss = loss_fn(f1, f2)
    loss.backward()
    opt.step()

for _ in range(3):
    step()
torch.cuda.synchronize()
lib = _lib.load()
runs = []
for _ in range(3):
    lib.focal_trace_begin(8192, _lib.TRACE_DISPATCH)
    step()
    torch.cuda.synchronize()
    lib.focal_trace_end()
    n = lib.focal_trace_count()
    recs = (_lib.TraceRecord * max(n, 1))()
    lib.focal_trace_read(0, n, recs)
    runs.append([(recs[i].kernel.decode(), list(recs[i].grid), list(recs[i].block), float(recs[i].us)) for i in range(n)])
last = runs[-1]
json.dump({"ape": ape, "root": root, "launches": last, "n": len(last), "sum_us": sum(r[3] for r in last)}, open(out, "w"))
emb = [r for r in last if "embed" in r[0] or "ape" in r[0]]
print(f"ape={ape} launches={len(last)} sum_us={sum(r[3] for r in last):.1f}")
for r in emb:
    print("  ", r[0][:90], r[1], f"{r[3]:.1f} us")
