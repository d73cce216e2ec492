#!/usr/bin/env python3
"""Training-step timing (forward in train mode + loss + backward + Adam) on synthetic crops:
tools/train_step.py [b] [N] [--optim torch|fused] [--autoclip [host|device]] [--chamfer chunked|fused] [--objective module|fused]
[--conv-wgrad rows|pairs] [--conv-dgrad conv|direct] [--pool modules|fused] [--norm modules|fused]
[--attention materialised|fused] [--dense modules|point_major] [--heads modules|kernels] [--conv-fwd tiles|compact] [--conv-fwd-all]
[--rotation host|device] [--wgrad fp32|split] [--wgrad-all] [--kernels]
--kernels: the all-kernels configuration in one flag -- Network(**DCL_Net.TRAIN_KERNELS) with --chamfer fused --objective fused
--optim fused --autoclip (the host form, unless --autoclip device is given); it overrides the single switches.  --rotation: Network(train_rotation=).
--optim fused: dcl.optim.Adam (csrc/optim.hip) instead of torch.optim.Adam; --autoclip: AutoClip(50) in front of the step, as
the reference's training scripts run it -- the per-tensor .item() form with --optim torch, dcl.optim.AutoClip with fused;
--autoclip device (needs --optim fused, or --kernels): dcl.optim.DeviceAutoClip, the history and the percentile on the GPU.
--chamfer / --objective: the loss module's switches (models/losses.py); --objective fused evaluates the objective on
csrc/objective.hip and logs all five loss values with one read-back of crit.packed.  --conv-wgrad: the form of the sparse
convolutions' weight gradient, Network(train_conv_wgrad=); --conv-dgrad: the form of their input gradient,
Network(train_conv_dgrad=); --pool: the form of the confidence-weighted pooling, Network(train_pool=); --norm: the form
of the backbones' BatchNorm1d + ReLU pairs, Network(train_norm=); --attention: the form of the correspondence attention,
Network(train_attention=); --dense: the layout of the dense half, Network(train_dense=) -- point_major needs --attention fused
and does not read --pool; --heads: the form of the heads' last layers and of the two pose heads, Network(train_heads=) -- kernels
needs --dense point_major; --conv-fwd: the form of the sparse convolutions' forward, Network(train_conv_fwd=) -- compact
runs on the widths of ops.CONV_FWD_COMPACT_WIDTHS; --conv-fwd-all (measurement only) puts all three dilating widths into that table
for this process, whatever was measured.  --wgrad: the form of the point-major dense half's weight gradients, Network(train_wgrad=)
-- split (needs --dense point_major, or --kernels, which leaves it alone) runs csrc/linear_wgrad_split.hip on the shapes of
ops.WGRAD_SPLIT_SHAPES; --wgrad-all (measurement only) makes that table name every shape for this process."""
import argparse, importlib, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
dcl = importlib.import_module("dcl-net_amd")
ap = argparse.ArgumentParser()
ap.add_argument("b", type=int, nargs="?", default=8)
ap.add_argument("n", type=int, nargs="?", default=1024)
ap.add_argument("--optim", choices=("torch", "fused"), default="torch")
ap.add_argument("--autoclip", nargs="?", const="host", default=None, choices=("host", "device"))
ap.add_argument("--chamfer", choices=("chunked", "fused"), default="chunked")
ap.add_argument("--objective", choices=("module", "fused"), default="module")
ap.add_argument("--conv-wgrad", choices=("rows", "pairs"), default="rows")
ap.add_argument("--conv-dgrad", choices=("conv", "direct"), default="conv")
ap.add_argument("--pool", choices=("modules", "fused"), default="modules")
ap.add_argument("--norm", choices=("modules", "fused"), default="modules")
ap.add_argument("--attention", choices=("materialised", "fused"), default="materialised")
ap.add_argument("--dense", choices=("modules", "point_major"), default="modules")
ap.add_argument("--heads", choices=("modules", "kernels"), default="modules")
ap.add_argument("--conv-fwd", choices=("tiles", "compact"), default="tiles")
ap.add_argument("--conv-fwd-all", action="store_true")
ap.add_argument("--rotation", choices=("host", "device"), default="host")
ap.add_argument("--wgrad", choices=("fp32", "split"), default="fp32")
ap.add_argument("--wgrad-all", action="store_true")
ap.add_argument("--kernels", action="store_true")
args = ap.parse_args()
b, n = args.b, args.n
switches = dict(train_conv_wgrad=args.conv_wgrad, train_conv_dgrad=args.conv_dgrad, train_pool=args.pool, train_norm=args.norm,
                train_attention=args.attention, train_dense=args.dense, train_heads=args.heads, train_conv_fwd=args.conv_fwd,
                train_rotation=args.rotation)
if args.kernels:
    switches = dict(dcl.DCL_Net.TRAIN_KERNELS)
    args.chamfer, args.objective, args.optim, args.autoclip = "fused", "fused", "fused", args.autoclip or "host"
if args.autoclip == "device" and args.optim != "fused":
    ap.error("--autoclip device needs --optim fused (or --kernels)")
switches["train_wgrad"] = args.wgrad
if args.wgrad_all:
    class _EveryShape(dict):
        get = lambda self, key, default=None: 0                                   # noqa: E731
        __repr__ = lambda self: "every shape"                                     # noqa: E731
    dcl.ops.WGRAD_SPLIT_SHAPES = _EveryShape()
if args.conv_fwd_all:
    dcl.ops.CONV_FWD_COMPACT_WIDTHS = frozenset(((32, 32), (64, 64), (128, 128)))
net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="train", **switches)
net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
net = net.cuda().train()
crit = dcl.DCL_Net.losses(None, chamfer=args.chamfer, objective=args.objective)
clip = None
if args.optim == "fused":
    opt = dcl.optim.Adam(net.parameters(), lr=1e-4)
    if args.autoclip:
        clip = (dcl.optim.DeviceAutoClip if args.autoclip == "device" else dcl.optim.AutoClip)(50, optimizer=opt)
else:
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    if args.autoclip:
        from bench_optim import ItemAutoClip
        clip = ItemAutoClip(50)
data = dcl.synth.make_batch(b, n, n)
data["flags"] = torch.zeros(b)
def step():
    opt.zero_grad()
    pred = net(data)
    loss = crit(pred, data["labels"])["loss_all"]
    loss.backward()
    if clip is not None: clip(net)
    opt.step()
    return loss
for _ in range(3): step()
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(10): l = step()
torch.cuda.synchronize()
print("train step b=%d N=M=%d (optim %s%s, chamfer %s, objective %s, conv fwd %s%s, wgrad %s, dgrad %s, linear wgrad %s%s, pool %s, norm %s, attention %s, dense %s, heads %s): %.1f ms (loss %.4f), peak mem %.2f GB" % (b, n, args.optim, " + autoclip (%s)" % args.autoclip if clip is not None else "", args.chamfer, args.objective, switches["train_conv_fwd"], " on %s" % sorted(dcl.ops.CONV_FWD_COMPACT_WIDTHS) if switches["train_conv_fwd"] == "compact" else "", switches["train_conv_wgrad"], switches["train_conv_dgrad"], switches["train_wgrad"], " on %r" % (dcl.ops.WGRAD_SPLIT_SHAPES,) if switches["train_wgrad"] == "split" else "", switches["train_pool"], switches["train_norm"], switches["train_attention"], switches["train_dense"], switches["train_heads"], (time.perf_counter() - t0) / 10 * 1e3, float(l.detach()), torch.cuda.max_memory_allocated() / 1e9))
if args.objective == "fused":
    print("  [loss_pose, loss_Xo, loss_Yc, loss_conf, loss_all] from one read-back: %s" % (["%.5f" % v for v in crit.packed.tolist()],))
