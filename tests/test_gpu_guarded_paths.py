"""Whole paths inside poisoned guard bands (tests/guard_arena.py): the eval forward launch by launch, the refiner, the refinement
loop, the crop builders and one all-kernels training step run plain and under both poisons with the allocation proxy installed
in every allocating module of the package.  Predictions, loss, gradients and updated parameters must have the same bits in all
three runs and every guard band must be intact.  The last test holds the op-level table of tests/test_gpu_guarded_ops.py to
what these paths enter."""
import random

import numpy as np
import pytest
import torch

import guard_arena as GA
import step_replay as SR
import test_gpu_guarded_ops as OPS

pytestmark = pytest.mark.gpu

CAPACITY = 1 << 30
CAPACITY_OF = {"train_step/2x256": 4 << 30}      # every sparse-conv call of the step takes a stream-K scratch of up to 64 MiB
ENTERED = {}          # path name -> the code objects of the allocating modules it entered (filled by whichever test runs first)


def _run(dcl, name, fn, compare=True):
    if OPS._FAULT:                               # shared with the op cases: nothing runs on the GPU after an error of the runtime
        pytest.fail("not run: %s ended in an error of the runtime" % OPS._FAULT[0])
    entered = set()
    mods = GA.allocating_modules(dcl)
    try:
        if compare:
            GA.guarded(fn, [], modules=mods, device="cuda", capacity=CAPACITY_OF.get(name, CAPACITY), entered=entered)
        else:
            GA.poison_pass(fn, [], "nan", modules=mods, device="cuda", capacity=CAPACITY_OF.get(name, CAPACITY), entered=entered)
    except AssertionError:
        raise
    except BaseException:
        OPS._FAULT.append(name)
        raise
    ENTERED[name] = entered
    torch.cuda.empty_cache()                     # the arenas are gone: hand their blocks back before the rest of the suite runs


# ---------------------------------------------------------------------------------------------------- the paths
def _eval_forward(dcl, b, n, m, cached):
    import test_gpu_template_cache as TT
    cfg = dcl.synth.default_cfg(n, m)
    sd = dcl.synth.synth_state_dict(dcl.DCL_Net.Network(cfg, mode="test"), 3)
    data = dcl.synth.make_batch(b, n, m, first=40)

    def fn():
        net = dcl.DCL_Net.Network(cfg, mode="test", graph_max_batch=0)          # launch by launch: nothing under graph capture
        net.load_state_dict(sd)
        net = net.cuda().eval()
        call = {k: ({kk: vv.clone() for kk, vv in v.items()} if isinstance(v, dict) else v) for k, v in data.items()}
        if cached:
            net.cache_templates(TT._templates(dcl, data["obj_idx"].tolist(), m), TT.LIMIT)
            call = TT._cached_call(call)
        with torch.no_grad():
            pred = net(call)
        return {k: v for k, v in pred.items() if torch.is_tensor(v)}
    return fn


def _refiner(dcl, seed=2):
    ref = dcl.refiner.Refiner()
    ref.load_state_dict(dcl.synth.synth_state_dict(ref, seed))
    return ref.cuda().eval()


def _refiner_eval(dcl):
    b, n = 3, 333
    g = torch.Generator().manual_seed(5)
    x = torch.randn(b, 259, n, generator=g).cuda()
    conf = torch.rand(b, n, generator=g).cuda()                            # one per point (the module reads conf[:, :1024])

    def fn():
        with torch.no_grad():
            out = _refiner(dcl)({"input_features": x.clone(), "conf": conf.clone(), "obj_idx": torch.zeros(b, dtype=torch.int64)})
        return {k: v for k, v in out.items() if torch.is_tensor(v)}
    return fn


def _refine_loop(dcl):
    import test_gpu_refine_loop as TR
    pred, pts = TR._loop_case(2, 256)

    def fn():
        with torch.no_grad():
            return dcl.refiner.refine_loop(_refiner(dcl, 4), {k: v.clone() for k, v in pred.items()}, pts.clone(), 2, compose="device",
                                           trajectory=True)
    return fn


def _data_tensors(data):
    return {k: v for k, v in data.items() if torch.is_tensor(v) or isinstance(v, dict)}


def _crops_eval(dcl, draws):
    import test_gpu_crops_device_draws as TD
    sc = TD._scene()

    def fn():
        np.random.seed(7)
        random.seed(7)
        kw = dict(draws="device", capacity=True, draw_seed=9) if draws == "device" else {}
        return _data_tensors(TD._builder(dcl, sc, **kw).build(*TD._args(dcl, sc)))
    return fn


def _crops_frames(dcl, draws):
    import test_gpu_frame_batches as TF
    scenes = TF._frames()

    def fn():
        np.random.seed(7)
        random.seed(7)
        kw = dict(draws="device", capacity=True, draw_seed=9) if draws == "device" else {}
        return _data_tensors(TF._builder(dcl, scenes, **kw).build_frames([TF._tuple(dcl, sc) for sc in scenes]))
    return fn


def _lmo_scenes():
    import lmo_scene as LM
    return [LM.make_lmo_scene(seed, tmp_size=LM.CFG["tmp_size"], **kw) for seed, kw in LM.CASES]


def _crops_lm(dcl, kind):
    """the LineMOD eval builders: one sample with the box from the mask (build_lm in eval mode, build_lmo), and the five scenes in
    one call with the draws on the device (build_lm_frames, build_lmo_frames)"""
    import test_gpu_lmo_crops as TL
    scs = _lmo_scenes()

    def fn():
        np.random.seed(7)
        random.seed(7)
        sc = scs[0]
        if kind == "build_lm":
            return TL._builder(dcl, sc).build_lm(sc["img"], sc["depth"], sc["mask_label"], None, sc["cls"], eval_mode=True)
        if kind == "build_lmo":
            return TL._builder(dcl, sc).build_lmo(sc["img"], sc["depth"], sc["mask_label"], sc["cls"])
        b = dcl.crops.CropBuilder(TL.CFG, sc["cad_pts"], sc["cad_col"], camera=dcl.crops.LM_CAMERA, draws="device", draw_seed=9)
        samples = [(c["img"], c["depth"], c["mask_label"], None, c["cls"]) for c in scs]
        return _data_tensors(b.build_lm_frames(samples, eval_mode=True) if kind == "build_lm_frames" else b.build_lmo_frames(samples))
    return fn


def _crops_train(dcl):
    import test_gpu_train_crops as TT
    import train_scene as TS
    sc, _ = TT.scene(TS.CASES[0][0])

    def fn():
        np.random.seed(7)
        random.seed(7)
        return _data_tensors(dcl.crops.CropBuilder(TS.CFG, sc["cad_pts"], sc["cad_col"]).build_train([TT.frame_of(sc)], [sc["meta"]]))
    return fn


def _crops_train_lm(dcl):
    import test_gpu_train_lm_crops as TL
    sc = TL.A.scene(TL.A.SEEDS[0])

    def fn():
        np.random.seed(7)
        random.seed(7)
        return _data_tensors(TL.lm_builder(dcl, sc).build_train_lm([TL.LS.sample_of(sc)]))
    return fn


def _train_step(dcl):
    def fn():
        net, out = SR.run_steps(dcl, 2, 256, steps=1)                          # TRAIN_KERNELS, fused Chamfer and objective, Adam + AutoClip
        return out[0]["loss"], out[0]["pred"], out[0]["grads"], {k: p.detach() for k, p in net.named_parameters()}
    return fn


PATHS = {
    "eval_forward/2x256x256": lambda dcl: _eval_forward(dcl, 2, 256, 256, False),
    "eval_forward/3x333x517": lambda dcl: _eval_forward(dcl, 3, 333, 517, False),
    "eval_forward/2x256x256/template_cache": lambda dcl: _eval_forward(dcl, 2, 256, 256, True),
    "eval_forward/3x333x517/template_cache": lambda dcl: _eval_forward(dcl, 3, 333, 517, True),
    "refiner_eval": _refiner_eval,
    "refine_loop/device": _refine_loop,
    "crops/build/host_draws": lambda dcl: _crops_eval(dcl, "host"),
    "crops/build/device_draws": lambda dcl: _crops_eval(dcl, "device"),
    "crops/build_frames/host_draws": lambda dcl: _crops_frames(dcl, "host"),
    "crops/build_frames/device_draws": lambda dcl: _crops_frames(dcl, "device"),
    "crops/build_lm": lambda dcl: _crops_lm(dcl, "build_lm"),
    "crops/build_lmo": lambda dcl: _crops_lm(dcl, "build_lmo"),
    "crops/build_lm_frames": lambda dcl: _crops_lm(dcl, "build_lm_frames"),
    "crops/build_lmo_frames": lambda dcl: _crops_lm(dcl, "build_lmo_frames"),
    "crops/build_train": _crops_train,
    "crops/build_train_lm": _crops_train_lm,
    "train_step/2x256": _train_step,
}


@pytest.mark.parametrize("name", list(PATHS))
def test_guarded_path(dcl, name):
    _run(dcl, name, PATHS[name](dcl))


# ---------------------------------------------------------------------------------------------------- coverage
# functions of ops.py that hold an uninitialised allocation, that the whole paths enter and that have no op-level case.  The
# only admissible reason: every tensor shape of the call is fixed by the network configuration, so there is no ragged edge to
# choose.
WHOLE_PATH_ONLY = {
}


def test_every_allocating_function_the_paths_enter_has_an_op_level_case(request, dcl):
    for name in PATHS:
        if name not in ENTERED:
            _run(dcl, name, PATHS[name](dcl), compare=False)
    by_case = set()
    for name in OPS.CASES:
        if OPS._FAULT:
            pytest.fail("not run: %s ended in an error of the runtime" % OPS._FAULT[0])
        try:
            OPS.run_case(dcl, request, name, compare=False, entered=by_case)
        except AssertionError:
            raise
        except BaseException:
            OPS._FAULT.append(name)
            raise
    ops = GA.allocating_modules(dcl)[0]
    allocating = set(GA.function_table(ops.__file__).allocating())
    names = lambda codes: GA.entered_names(codes, ops)                                                     # noqa: E731
    op_level = names(by_case)
    # the censuses are not empty: functions every run of either kind is known to enter
    assert {"sparse_conv", "cross_attention", "_layer_io", "crop_points_frames", "crop_draw_keyed"} <= op_level, sorted(op_level)
    assert set(ENTERED) == set(PATHS)
    assert "sparse_conv" in names(ENTERED["train_step/2x256"]) and "pose_heads_parts" in names(ENTERED["eval_forward/2x256x256"])
    assert "crop_draw_keyed" in names(ENTERED["crops/build_frames/device_draws"])
    assert len(allocating) > 60 and "sparse_conv" in allocating
    missing = {}
    for path, codes in ENTERED.items():
        for fn in sorted((names(codes) & allocating) - op_level - set(WHOLE_PATH_ONLY)):
            missing.setdefault(fn, []).append(path)
    assert not missing, "functions of ops.py with an uninitialised allocation that only whole paths enter:\n" + "\n".join(
        "  %s (%s)" % (fn, ", ".join(paths)) for fn, paths in sorted(missing.items()))
    stale = sorted(fn for fn in WHOLE_PATH_ONLY if fn in op_level or fn not in allocating)
    assert not stale, "WHOLE_PATH_ONLY entries that have an op-level case or allocate nothing: %s" % stale
