"""Generates tests/golden/lmo_metric_ref.npz with the REFERENCE's own Occlusion-LineMOD metric code: the body of the eval
loop in tools/test_LMO.py (:104-156) -- the lost-frame branch that counts a lost detection into num_count ("Following
HybridPose, count it on", :104-118) and, for the other frames, ADD / ADD-S, `dis < diameter[idx]`, success_count / num_count
-- executed from the reference source where make_lm_metric_golden.py finds it (nothing is copied): the statements are
compiled out of the script's AST as make_lm_metric_golden.py does, here as the body of a loop over one frame at a time
(the branch ends in `continue`), and fed seeded poses; `model(data)` returns the frame's seeded prediction and `.cuda()` is
a no-op.  8 objects, frames of one object each, some of them lost.

    python tests/golden/make_lmo_metric_golden.py
"""
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_lm_metric_golden import SRC as LM_SRC, _Sink, rand_rot  # noqa: E402

SRC = os.path.join(os.path.dirname(LM_SRC), "test_LMO.py")
SYM_IDX = (5, 6)                                                       # LM/dataloader_test_LMO.py:104


def loop_code():
    """`for data in frames:` around the statements of `for i, data in enumerate(dataloder)` up to the progress-bar text"""
    tree = ast.parse(open(SRC).read())
    test = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "test"][0]
    loop = [n for w in ast.walk(test) if isinstance(w, ast.With) for n in w.body if isinstance(n, ast.For)][0]
    keep = []
    for st in loop.body:
        if ast.unparse(st).startswith("t.set_description"):
            break
        keep.append(st)
    assert ast.unparse(keep[0]).startswith("if data['flags'].shape[0] == 1 and"), ast.unparse(keep[0])[:80]
    outer = ast.For(target=ast.Name(id="data", ctx=ast.Store()), iter=ast.Name(id="frames", ctx=ast.Load()), body=keep,
                    orelse=[])
    return compile(ast.fix_missing_locations(ast.Module(body=[outer], type_ignores=[])), SRC, "exec")


class _Bar(object):
    def update(self, *_):
        pass


def main():
    torch.Tensor.cuda = lambda self, *a, **k: self
    code = loop_code()
    rng = np.random.default_rng(17)
    n_obj, P, frames = 8, 160, 80
    diameter = (rng.uniform(0.1, 0.3, n_obj) * 0.1).tolist()              # metres * 0.1, as tools/test_LMO.py:70-73 forms them

    class Cfg(object):
        pass
    cfg = Cfg()
    cfg.diameter, cfg.num_objects = diameter, n_obj
    ns = {"torch": torch, "np": np, "cfg": cfg, "fw": _Sink(), "t": _Bar(), "count": 0, "model": lambda d: d["pred"],
          "success_count": [0] * n_obj, "num_count": [0] * n_obj}
    out = {"diameter": np.array(diameter, np.float64), "n_frames": np.array([frames])}
    clouds = (rng.normal(size=(n_obj, P, 3)) * rng.uniform(0.02, 0.06, (n_obj, 1, 1))).astype(np.float32)
    out["clouds"] = clouds
    lost = 0
    for f in range(frames):
        idx = rng.integers(0, n_obj, 1)
        flag = -1 if rng.random() < 0.2 else int(int(idx[0]) in SYM_IDX)
        flags = np.array([flag], np.int64)
        Rg = np.stack([rand_rot(rng)])
        tg = rng.normal(0, 0.3, (1, 3)).astype(np.float32)
        scale = rng.choice([0.01, 0.05, 0.2, 1.0], size=1)
        Rp = np.stack([rand_rot(rng, s) @ R for s, R in zip(scale, Rg)]).astype(np.float32)
        tp = (tg + rng.normal(0, 0.004, (1, 3)) * scale[:, None] * 5).astype(np.float32)
        if flag == -1:                      # the loader's collate for a frame without a sample: flags, obj_idx, gt pose only
            lost += 1
            data = {"flags": torch.from_numpy(flags).float(), "obj_idx": torch.from_numpy(idx.astype(np.int32)),
                    "rot_gt": torch.from_numpy(Rg), "trans_gt": torch.from_numpy(tg)}
        else:
            data = {"labels": {"points_tmp": torch.from_numpy(clouds[idx]), "rot_gt": torch.from_numpy(Rg),
                               "trans_gt": torch.from_numpy(tg)},
                    "flags": torch.from_numpy(flags).float(), "obj_idx": torch.from_numpy(idx.astype(np.int32)),
                    "pred": {"rot_pred": torch.from_numpy(Rp), "trans_pred": torch.from_numpy(tp)}}
        ns["frames"] = [data]
        ns.pop("l2_dis", None)
        exec(code, ns)
        out["f%d_flags" % f], out["f%d_idx" % f] = flags.astype(np.int32), idx.astype(np.int32)
        out["f%d_Rp" % f], out["f%d_tp" % f], out["f%d_Rg" % f], out["f%d_tg" % f] = Rp, tp, Rg, tg
        if flag != -1:
            out["f%d_l2" % f], out["f%d_cd" % f] = ns["l2_dis"].numpy(), ns["cd_dis"].numpy()
        else:
            assert "l2_dis" not in ns
            out["f%d_l2" % f] = out["f%d_cd" % f] = np.zeros(0, np.float32)
    assert 5 <= lost <= frames // 2
    out["success_count"] = np.array(ns["success_count"], np.int64)
    out["num_count"] = np.array(ns["num_count"], np.int64)
    out["count"] = np.array([ns["count"]], np.int64)
    assert int(out["num_count"].sum()) == frames                          # lost frames are counted
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "lmo_metric_ref.npz"), **out)
    print("golden written: lmo_metric_ref.npz  success", out["success_count"].tolist(), "of", out["num_count"].tolist(),
          "lost", lost, "reference's count", int(out["count"][0]))


if __name__ == "__main__":
    main()
