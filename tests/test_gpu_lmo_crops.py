"""The Occlusion-LineMOD sample builder on the device: CropBuilder.build_lmo against the reference loader's own outputs
(tests/golden/lmo_crops_ref.npz, made by tests/golden/make_lmo_crops_golden.py from LM/dataloader_test_LMO.py) bit for
bit; the mask-derived box of build_lm(obj_bb=None); and one sample through Network, add_lm and LmoTable."""
import os

import numpy as np
import pytest
import torch

from lmo_scene import CASES, CFG, make_lmo_scene

pytestmark = pytest.mark.gpu

KEYS = ("feat_inp", "vox_inp", "feat_tmp", "vox_tmp", "centroid")


def _builder(dcl, sc, cfg=CFG):
    return dcl.crops.CropBuilder(cfg, sc["cad_pts"], sc["cad_col"], camera=dcl.crops.LM_CAMERA)


def test_build_lmo_equals_the_reference_loader(dcl, golden_dir):
    z = np.load(os.path.join(golden_dir, "lmo_crops_ref.npz"))
    dummies = 0
    for seed, kw in CASES:
        sc = make_lmo_scene(seed, tmp_size=CFG["tmp_size"], **kw)
        tag = "lmo%d_" % seed
        # the box and the crop rows the reference's own mask_to_bbox / get_bbox returned
        mb = dcl.ops.mask_box(torch.from_numpy(sc["mask_label"].astype(np.int32)).cuda(), 1, 0).cpu().numpy()[0]
        assert mb[:4].tolist() == z[tag + "box"].tolist() and mb[4:8].tolist() == z[tag + "crop"].tolist(), tag
        np.random.seed(seed)
        got = _builder(dcl, sc).build_lmo(sc["img"], sc["depth"], sc["mask_label"], sc["cls"])
        if float(z[tag + "flag"][0]) == -1:
            assert got is None, tag
            dummies += 1
            continue
        assert got is not None, tag
        for g, k in zip(got, KEYS):
            assert np.array_equal(g.cpu().numpy(), z[tag + k]), (tag, k)
    assert dummies == 2                                                      # depth 0 under the whole mask; empty mask


@pytest.mark.parametrize("seed,kw", CASES[:3])
def test_build_lm_takes_the_box_from_the_mask_when_none_is_given(dcl, seed, kw):
    """build_lm(obj_bb=None, eval_mode=True) == build_lm(obj_bb=box) with the box of the host twin on the same mask"""
    sc = make_lmo_scene(seed, tmp_size=CFG["tmp_size"], **kw)
    b = _builder(dcl, sc)
    box = dcl.ops.mask_box_host(sc["mask_label"], 1, 0)[0][:4].tolist()
    np.random.seed(seed)
    want = b.build_lm(sc["img"], sc["depth"], sc["mask_label"], box, sc["cls"], True)
    np.random.seed(seed)
    got = b.build_lm(sc["img"], sc["depth"], sc["mask_label"], None, sc["cls"], eval_mode=True)
    assert want is not None and got is not None
    for g, w in zip(got, want):
        assert torch.equal(g, w)


def test_one_lmo_sample_runs_through_the_network_and_the_table(dcl):
    cfg = dict(CFG, input_size=256, tmp_size=256)
    seed, kw = CASES[0]
    sc = make_lmo_scene(seed, tmp_size=256, **kw)
    for c in sc["cad_pts"]:
        sc["cad_pts"][c] = sc["cad_pts"][c] * 0.8
    np.random.seed(3)
    feat_inp, vox_inp, feat_tmp, vox_tmp, centroid = _builder(dcl, sc, cfg).build_lmo(sc["img"], sc["depth"], sc["mask_label"],
                                                                                       sc["cls"])
    S, mode = int(cfg["voxel_num_limit"][0]), cfg["voxelization_mode"]
    data = {"labels": {}, "batch_offsets": (torch.arange(2) * cfg["input_size"]).int(), "voxel_num_limit": torch.tensor([S, S, S]),
            "flags": torch.IntTensor([0]), "obj_idx": torch.IntTensor([2])}
    for side, feats, vox in (("inp", feat_inp, vox_inp), ("tmp", feat_tmp, vox_tmp)):       # the loader's collate, b = 1
        coords = torch.cat([torch.zeros((vox.shape[0], 1), dtype=torch.int64, device=vox.device), vox], 1).contiguous()
        occ, p2v, v2p = dcl.ops.voxelize_idx_gpu(coords, 1, S, mode)
        data[side] = {"feats": feats, "occupied_voxels": occ, "p2v_maps": p2v, "v2p_maps": v2p}
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(256, 256, unit=0.005), mode="test", graph_max_batch=0)
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.cuda().eval()
    with torch.no_grad():
        pred = net(data)
    assert pred["rot_pred"].shape == (1, 3, 3) and torch.isfinite(pred["rot_pred"]).all() and torch.isfinite(pred["trans_pred"]).all()
    R_gt = torch.eye(3, device="cuda").unsqueeze(0)
    t_gt = (torch.tensor([[0.01, 0.02, 0.8]], device="cuda") - centroid.unsqueeze(0)).float()
    dis = dcl.sharding.add_lm(data["labels"]["points_tmp"], pred["rot_pred"], pred["trans_pred"], R_gt, t_gt,
                              torch.zeros(1, dtype=torch.int32, device="cuda"))
    assert dis.shape == (1,) and bool(torch.isfinite(dis).all())
    table = dcl.sharding.LmoTable([0.01] * 8)
    table.add_batch(data["obj_idx"].tolist(), dis.tolist(), data["flags"].tolist())
    table.add_batch([4], [], [-1])                                           # and a frame whose detection was lost
    assert table.counts[:, 0].tolist() == [0, 0, 1, 0, 1, 0, 0, 0] and int(table.counts[4, 1]) == 0
