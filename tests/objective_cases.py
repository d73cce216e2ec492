"""Cases, float64 references and error bounds shared by tests/test_objective_host.py and tests/test_gpu_objective.py.

Every reference is evaluated in float64 on the SAME fp32 arrays the code under test receives, so conditioning does not enter
a bound.  eps = 2^-24 is the unit round-off of fp32; an fp32 operation has relative error <= eps, logf <= 1 ulp = 2 eps.
A case is built once per (shape, sym pattern) and cached; nobody modifies it."""
import functools
import math

import torch

EPS = 2.0 ** -24
SHAPES = [(1, 1), (3, 63), (3, 65), (2, 257), (5, 1024)]
SYM_KINDS = ["zeros", "ones", "mixed"]
UPSTREAM = ["all", "pose", "random"]
LANES = 256

# Constant of the scalar bound (C_SUM + ceil(n/256) + b) * eps, derived from the pinned order (include/dclnet_hip.h):
#   a per-point term LXo / LYc / pose carries <= 6 eps (bound below); a conf term L c - 0.01 log c is a sum of two non-negative
#   parts: L c <= 7 eps, 0.01 log c <= 2 (logf, 1 ulp) + 1 (the fp32 constant 0.01f) + 1 (product) = 4 eps, their sum + 1: 8 eps;
#   a lane adds ceil(n/256) terms: ceil(n/256) - 1 further roundings (its first add, to 0, is exact);  the fold has 8 levels: 8;
#   the crops are added ascending: b - 1;  loss_conf adds its two halves: 1;  the division by the count: 1;
#   loss_all = ((pose + 5 Xo) + Yc) + conf: one product and three sums of non-negative numbers: 4.
# Total for loss_all, the largest: 8 + (ceil(n/256) - 1) + 8 + (b - 1) + 1 + 1 + 4 = ceil(n/256) + b + 20.
C_SUM = 20


def scalar_bound(b, n):
    bound = (C_SUM + math.ceil(n / LANES) + b) * EPS
    assert bound <= 128 * EPS, "a bound looser than 128 eps means the summation order is not the one the header pins"
    return bound


def sym_flags(b, kind):
    if kind == "zeros":
        return torch.zeros(b)
    if kind == "ones":
        return torch.ones(b)
    return (torch.arange(b) % 2).float() if b > 1 else torch.ones(1)


def rand_rot(g, b):
    q, _ = torch.linalg.qr(torch.randn(b, 3, 3, generator=g, dtype=torch.float64))
    return q


def rigid64(p, R, t, inverse):
    """the formula in float64: R p + t, or R^T (p - t)"""
    p, R, t = p.double(), R.double(), t.double()
    return torch.bmm(p - t.unsqueeze(1), R) if inverse else torch.bmm(p, R.transpose(1, 2)) + t.unsqueeze(1)


def chamfer64(pred, target):
    """both halves of the literal Chamfer formula in float64, and the argmins"""
    d = torch.norm(pred.double().unsqueeze(2) - target.double().unsqueeze(1), dim=3)
    pt, ipt = d.min(dim=2)
    tp, itp = d.min(dim=1)
    return pt, tp, ipt, itp


@functools.lru_cache(maxsize=None)
def case(b, n, kind, seed=0):
    """fp32 CPU inputs of one objective call.  The clouds come from the float64 rigid formula rounded to fp32, the Chamfer
    halves from the literal float64 formula rounded to fp32; every crop has one point at distance exactly 0 in each L2 term."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * b + n)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)                        # noqa: E731
    tmp, inp = rn(b, n, 3) * 0.05, rn(b, n, 3) * 0.05
    R, R_gt = rand_rot(g, b), rand_rot(g, b)
    t, t_gt = rn(b, 3) * 0.01, rn(b, 3) * 0.01
    c = {"tmp": tmp.float(), "inp": inp.float(), "R": R.float(), "t": t.float(), "R_gt": R_gt.float(), "t_gt": t_gt.float()}
    c["posed"] = rigid64(c["tmp"], c["R"], c["t"], False).float()
    c["posed_gt"] = rigid64(c["tmp"], c["R_gt"], c["t_gt"], False).float()
    c["cano_pred"] = rigid64(c["inp"], c["R"], c["t"], True).float()
    c["cano_gt"] = rigid64(c["inp"], c["R_gt"], c["t_gt"], True).float()
    c["Xo"] = (c["cano_gt"].double() + rn(b, n, 3) * 0.01).float()
    c["Yc"] = (c["posed_gt"].double() + rn(b, n, 3) * 0.01).float()
    c["conf"] = (torch.rand(b, 2 * n, generator=g, dtype=torch.float64) * 0.8 + 0.1).float()
    c["sym"] = sym_flags(b, kind)
    i = [k % n for k in range(5)]
    c["posed"][:, i[0]] = c["posed_gt"][:, i[0]]
    c["Xo"][:, i[1]] = c["cano_gt"][:, i[1]]
    c["Xo"][:, i[2]] = c["cano_pred"][:, i[2]]
    c["Yc"][:, i[3]] = c["posed_gt"][:, i[3]]
    c["Yc"][:, i[4]] = c["posed"][:, i[4]]
    for name, (p, q) in {"cd_pose": ("posed", "posed_gt"), "cd_Xo": ("Xo", "tmp"), "cd_Yc": ("Yc", "posed_gt")}.items():
        pt, tp, _, _ = chamfer64(c[p], c[q])
        live = (c["sym"] != 0).double().unsqueeze(1)                                         # a crop whose flag is 0 is not computed
        c[name] = ((pt * live).float().contiguous(), (tp * live).float().contiguous())
    c["g_random"] = torch.randn(5, generator=g)
    c["g_out"] = torch.randn(b, n, 3, generator=g)
    return {k: (v.contiguous() if torch.is_tensor(v) else v) for k, v in c.items()}


def objective_args(c, full=True):
    """positional + keyword arguments of ops.pose_objective(_host) for a case"""
    args = (c["posed"], c["posed_gt"], c["sym"], c["cd_pose"])
    kw = dict(Yc=c["Yc"], cano_pred=c["cano_pred"], cano_gt=c["cano_gt"], Xo=c["Xo"], conf=c["conf"], cd_Xo=c["cd_Xo"],
              cd_Yc=c["cd_Yc"]) if full else {}
    return args, kw


def backward_args(c, g_packed, L, full=True):
    args = (g_packed, c["posed"], c["posed_gt"], c["sym"])
    kw = dict(Yc=c["Yc"], cano_pred=c["cano_pred"], cano_gt=c["cano_gt"], Xo=c["Xo"], conf=c["conf"], L=L) if full else {}
    return args, kw


def upstream(c, kind):
    if kind == "all":
        return torch.tensor([0.0, 0.0, 0.0, 0.0, 1.0])
    if kind == "pose":
        return torch.tensor([1.0, 0.0, 0.0, 0.0, 0.0])
    return c["g_random"].clone()


def to(c, device):
    return {k: (v.to(device) if torch.is_tensor(v) else tuple(x.to(device) for x in v)) for k, v in c.items()}


def forward64(c, leaves=None, full=True):
    """the formulas of losses.forward in float64 on the case's fp32 arrays -> dict(dists, L, packed).  `leaves` replaces the
    differentiable inputs by float64 leaf tensors (the backward reference)."""
    v = {k: (x.double() if torch.is_tensor(x) else tuple(y.double() for y in x)) for k, x in c.items()}
    if leaves:
        v.update(leaves)
    b, n = v["posed"].shape[:2]
    s = v["sym"].unsqueeze(1)
    L2 = lambda a, d: torch.norm(a - d, dim=2)                                               # noqa: E731
    cd = lambda h: 0.5 * (h[0] + h[1])                                                       # noqa: E731
    dist = {"pose": L2(v["posed"], v["posed_gt"])}
    pose = (1 - s) * dist["pose"] + s * cd(v["cd_pose"])
    loss_pose = pose.sum() / (b * n)
    if not full:
        return {"dist": dist, "packed": torch.stack([loss_pose, loss_pose * 0, loss_pose * 0, loss_pose * 0, loss_pose])}
    dist.update(Xo_gt=L2(v["Xo"], v["cano_gt"]), Xo_pred=L2(v["Xo"], v["cano_pred"]), Yc_gt=L2(v["Yc"], v["posed_gt"]),
                Yc_posed=L2(v["Yc"], v["posed"].detach()))
    LXo = (1 - s) * dist["Xo_gt"] + 0.5 * s * (cd(v["cd_Xo"]) + dist["Xo_pred"])
    LYc = (1 - s) * dist["Yc_gt"] + 0.5 * s * (cd(v["cd_Yc"]) + dist["Yc_posed"])
    L = torch.cat([LXo, LYc], dim=1)
    loss_conf = (L.detach() * v["conf"] - 0.01 * torch.log(v["conf"])).sum() / (2 * b * n)
    loss_Xo, loss_Yc = LXo.sum() / (b * n), LYc.sum() / (b * n)
    return {"dist": dist, "L": L, "packed": torch.stack([loss_pose, loss_Xo, loss_Yc, loss_conf,
                                                         loss_pose + 5 * loss_Xo + loss_Yc + loss_conf])}


def backward64(c, g_packed, full=True):
    """float64 gradients of <g_packed, packed> with respect to posed, Xo, Yc, conf and the six Chamfer halves (autograd on
    forward64: torch.norm's backward gives 0 at distance 0)"""
    names = ["posed"] + (["Xo", "Yc", "conf"] if full else [])
    leaves = {k: c[k].double().requires_grad_() for k in names}
    for k in ["cd_pose"] + (["cd_Xo", "cd_Yc"] if full else []):
        leaves[k] = tuple(h.double().requires_grad_() for h in c[k])
    out = forward64(c, leaves, full)["packed"]
    (out * g_packed.double()).sum().backward()
    z = lambda x: torch.zeros_like(x) if x.grad is None else x.grad                          # noqa: E731
    return {k: (z(x) if torch.is_tensor(x) else tuple(z(h) for h in x)) for k, x in leaves.items()}


def weights_abs(g_packed, b, n):
    """|weight| of each gradient: the sum of the magnitudes the device weight is formed from, over the count -- equal to |W|
    unless the upstream entries cancel, where no fp32 sum is relatively accurate"""
    g = g_packed.double().abs()
    return {"pose": float(g[0] + g[4]) / (b * n), "Xo": float(g[1] + 5 * g[4]) / (b * n), "Yc": float(g[2] + g[4]) / (b * n),
            "conf": float(g[3] + g[4]) / (2 * b * n)}


def rigid_grad_bounds(c, inverse):
    """component-wise (ceil(n/256) + 10) eps sum_i |g_i| |p_i| for g_R and g_t, evaluated in float64.  The magnitudes are
    those of the products the sum is made of: forward form g_R[r][c] = sum g_r p_c, g_t[r] = sum g_r (|p| = 1); inverse form
    g_R[r][c] = sum q_r g_c with |q| <= |p| + |t|, g_t[r] = -sum (R g)_r with |(R g)_r| <= (|R| |g|)_r."""
    p, g, R, t = c["tmp"].double().abs(), c["g_out"].double().abs(), c["R"].double().abs(), c["t"].double().abs()
    n = p.shape[1]
    k = (math.ceil(n / LANES) + 10) * EPS
    if not inverse:
        return k * torch.einsum("bnr,bnc->brc", g, p), k * g.sum(dim=1)
    q = p + t.unsqueeze(1)
    return k * torch.einsum("bnr,bnc->brc", q, g), k * torch.einsum("brc,bnc->br", R, g)


# ---- the loss modules end to end ----------------------------------------------------------------------------------------
MODULE_SEED = {"losses": 0, "refiner": 3}                 # the first seeds whose clouds meet gap_ok (float64, no GPU needed)
GAP = 1e-5


def module_case(which, seed=None):
    """fp32 CPU inputs of losses (b = 4, n = m = 256, sym = [0,1,0,1]) or losses_refiner (a (3, 2620, 3) cloud, sym = [0,1,0]):
    Gaussian clouds of scale 0.05, random rotations"""
    seed = MODULE_SEED[which] if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)                                             # noqa: E731
    rot = lambda b: rand_rot(g, b).float()                                                   # noqa: E731
    if which == "losses":
        b, n = 4, 256
        pred = {"rot_pred": rot(b), "trans_pred": rn(b, 3) * 0.01, "sym_flag": torch.tensor([0.0, 1.0, 0.0, 1.0]),
                "conf": torch.rand(b, 2 * n, generator=g) * 0.8 + 0.1, "Xo_pred": rn(b, n, 3) * 0.05, "Yc_pred": rn(b, n, 3) * 0.05}
        gt = {"rot_gt": rot(b), "trans_gt": rn(b, 3) * 0.01, "points_tmp": rn(b, n, 3) * 0.05, "points_inp": rn(b, n, 3) * 0.05}
        return pred, gt
    b, n = 3, 2620
    pred = {"rot_pred": rot(b), "trans_pred": rn(b, 3) * 0.01}
    extra = {"trans_cur": rn(b, 3) * 0.01, "rot_cur": rot(b), "points_tmp": rn(b, n, 3) * 0.05,
             "sym_flag": torch.tensor([0.0, 1.0, 0.0])}
    gt = {"rot_gt": rot(b), "trans_gt": rn(b, 3) * 0.01}
    return pred, extra, gt


def chamfer_pairs64(which, case_):
    """the (pred, target) clouds of the module's Chamfer calls, in float64 from the fp32 inputs"""
    if which == "losses":
        pred, gt = case_
        posed = rigid64(gt["points_tmp"], pred["rot_pred"], pred["trans_pred"], False)
        posed_gt = rigid64(gt["points_tmp"], gt["rot_gt"], gt["trans_gt"], False)
        return [(posed, posed_gt), (pred["Xo_pred"].double(), gt["points_tmp"].double()), (pred["Yc_pred"].double(), posed_gt)]
    pred, extra, gt = case_
    delta = rigid64(extra["points_tmp"], pred["rot_pred"], pred["trans_pred"], False)
    refined = rigid64(delta, extra["rot_cur"], extra["trans_cur"], False)
    return [(refined, rigid64(extra["points_tmp"], gt["rot_gt"], gt["trans_gt"], False))]


def nearest_gap(pred, target):
    """smallest relative gap (second - nearest) / second over every point of both directions, and the float64 argmins"""
    worst, idx = 1.0, []
    for axis in (2, 1):
        best = []
        for c in range(pred.shape[0]):                    # crop by crop: the (n, m) matrix of one crop at a time
            d = torch.norm(pred[c].unsqueeze(1) - target[c].unsqueeze(0), dim=2)
            two, where = torch.topk(d, 2, dim=axis - 1, largest=False)
            two, where = (two, where) if axis == 2 else (two.t(), where.t())
            worst = min(worst, float(((two[:, 1] - two[:, 0]) / two[:, 1]).min()))
            best.append(where[:, 0])
        idx.append(torch.stack(best))
    return worst, idx[0], idx[1]


def gap_ok(which, seed):
    return all(nearest_gap(p, t)[0] >= GAP for p, t in chamfer_pairs64(which, module_case(which, seed)))


# ---- the same formulas in a dtype (tests/test_gpu_step_replay.py: the operands of a call recorded inside the network) -----------
def objective_form(c, g_packed, dtype):
    """forward64 / backward64 with every array in `dtype` (full form): float64 is the reference, float32 the module form, the
    torch composition of models/losses.py on the Chamfer halves as given -> dict(packed, posed, Xo, Yc, conf, cd_pose, cd_Xo,
    cd_Yc), the last seven the gradients of <g_packed, packed>, the cd_* as (pt, tp) pairs"""
    v = {k: (x.to(dtype) if torch.is_tensor(x) else tuple(y.to(dtype) for y in x)) for k, x in c.items()}
    leaves = {k: v[k].clone().requires_grad_() for k in ("posed", "Xo", "Yc", "conf")}
    for k in ("cd_pose", "cd_Xo", "cd_Yc"):
        leaves[k] = tuple(h.clone().requires_grad_() for h in v[k])
    v.update(leaves)
    b, n = v["posed"].shape[:2]
    s = v["sym"].unsqueeze(1)
    L2 = lambda a, d: torch.norm(a - d, dim=2)                                               # noqa: E731
    cd = lambda h: 0.5 * (h[0] + h[1])                                                       # noqa: E731
    pose = (1 - s) * L2(v["posed"], v["posed_gt"]) + s * cd(v["cd_pose"])
    LXo = (1 - s) * L2(v["Xo"], v["cano_gt"]) + 0.5 * s * (cd(v["cd_Xo"]) + L2(v["Xo"], v["cano_pred"]))
    LYc = (1 - s) * L2(v["Yc"], v["posed_gt"]) + 0.5 * s * (cd(v["cd_Yc"]) + L2(v["Yc"], v["posed"].detach()))
    L = torch.cat([LXo, LYc], dim=1)
    loss_conf = (L.detach() * v["conf"] - 0.01 * torch.log(v["conf"])).sum() / (2 * b * n)
    loss_pose, loss_Xo, loss_Yc = pose.sum() / (b * n), LXo.sum() / (b * n), LYc.sum() / (b * n)
    packed = torch.stack([loss_pose, loss_Xo, loss_Yc, loss_conf, loss_pose + 5 * loss_Xo + loss_Yc + loss_conf])
    (packed * g_packed.to(dtype)).sum().backward()
    z = lambda x: torch.zeros_like(x) if x.grad is None else x.grad                          # noqa: E731
    out = {k: (z(x) if torch.is_tensor(x) else tuple(z(h) for h in x)) for k, x in leaves.items()}
    out["packed"] = packed.detach()
    return out
