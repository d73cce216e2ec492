"""The per-class template cache of the eval forward (Network.cache_templates, data["tmp_cls"]): a call that carries class ids and
NO data["tmp"] against the oracle graph on the full data, at the project's own tolerances (tests/test_gpu_network.py: |dR| <=
1e-4, |dt| <= 1e-5, |dconf| <= 1e-4, F_Xo_p within 1e-4 max(1, max|ref|)), launch by launch and under default routing; the
entries' independence of their neighbours; the cache following the weights; the routing; the refusals; the crop builder."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

R_TOL, T_TOL, C_TOL, F_TOL = 1e-4, 1e-5, 1e-4, 1e-4
LIMIT = [64, 64, 64]


def _network(dcl, n_inp, n_tmp, unit=0.006, sd=None, **kw):
    cfg = dcl.synth.default_cfg(n_inp, n_tmp, unit)
    net = dcl.DCL_Net.Network(cfg, mode="test", **kw)
    sd = dcl.synth.synth_state_dict(net, 3) if sd is None else sd
    net.load_state_dict(sd)
    return net.cuda().eval(), sd, cfg


def _templates(dcl, classes, n_tmp, unit=0.006):
    return {int(c): dcl.synth.class_template_side(int(c), n_tmp, unit) for c in sorted(set(int(c) for c in classes))}


def _cached_call(data, ids=None):
    """the call's data with class ids in place of the template side"""
    out = {k: v for k, v in data.items() if k != "tmp"}
    out["labels"] = dict(data["labels"])
    out["tmp_cls"] = data["obj_idx"].tolist() if ids is None else ids
    return out


def _close(pred, want):
    dR = float((pred["rot_pred"].cpu() - want["rot_pred"].cpu()).abs().max())
    dt = float((pred["trans_pred"].cpu() - want["trans_pred"].cpu()).abs().max())
    dc = float((pred["conf"].cpu() - want["conf"].cpu()).abs().max())
    wF = want["F_Xo_p"].cpu()
    dF = float((pred["F_Xo_p"].cpu() - wF).abs().max())
    capF = F_TOL * max(1.0, float(wF.abs().max()))
    print("|dR| %.3g (tol %.0e)  |dt| %.3g (tol %.0e)  |dconf| %.3g (tol %.0e)  |dF| %.3g (tol %.3g)"
          % (dR, R_TOL, dt, T_TOL, dc, C_TOL, dF, capF))
    assert dR <= R_TOL and dt <= T_TOL and dc <= C_TOL and dF <= capF


_ORACLE = {}


def _oracle_forward(dcl, shape):
    """oracle.graph.forward on the FULL data of a shape, once"""
    if shape not in _ORACLE:
        from oracle import graph as G
        b, n_inp, n_tmp, unit = shape
        cfg = dcl.synth.default_cfg(n_inp, n_tmp, unit)
        net = dcl.DCL_Net.Network(cfg, mode="test")
        sd = dcl.synth.synth_state_dict(net, 3)
        data = dcl.synth.make_batch(b, n_inp, n_tmp, unit=unit, first=40)
        ref = {k: ({kk: vv.clone() for kk, vv in v.items()} if isinstance(v, dict) else v) for k, v in data.items()}
        _ORACLE[shape] = (sd, data, G.forward(sd, dict(cfg), ref, mode="test"))
    return _ORACLE[shape]


# ------------------------------------------------------------------------------------------- 1. against the oracle graph
@pytest.mark.parametrize("routing", ["launch by launch", "default"])
@pytest.mark.parametrize("shape", [(3, 256, 256, 0.006), (2, 333, 517, 0.006), (1, 1024, 1024, 0.005), (9, 256, 256, 0.006)],
                         ids=lambda s: "b%d-n%d-m%d-u%g" % s)
def test_cached_forward_matches_the_oracle_graph(dcl, oracle, shape, routing):
    b, n_inp, n_tmp, unit = shape
    sd, data, want = _oracle_forward(dcl, shape)
    kw = {"graph_max_batch": 0} if routing == "launch by launch" else {}
    net, _, _ = _network(dcl, n_inp, n_tmp, unit, sd=sd, **kw)
    cache = net.cache_templates(_templates(dcl, data["obj_idx"].tolist(), n_tmp, unit), LIMIT)
    assert tuple(cache.rows.shape) == (len(cache.class_ids), n_tmp, 643) and cache.rows.data_ptr() % 16 == 0
    call = _cached_call(data)
    assert "tmp" not in call
    with torch.no_grad():
        pred = net(call)
    # (nine crops are past graph_max_batch = 8; a default network still replays a graph while b (N + M) <= graph_max_points)
    graphs = 1 if routing == "default" and net.replays_graph(b) else 0
    assert len(net.__dict__.get("_graphs", {})) == graphs
    _close(pred, want)
    xyz = data["tmp"]["feats"][:, 4:7].reshape(b, n_tmp, 3)
    assert torch.equal(call["labels"]["points_tmp"].cpu(), xyz)                          # the templates' xyz, exactly
    assert torch.equal(call["labels"]["points_inp"].cpu(), data["inp"]["feats"][:, 4:7].reshape(b, n_inp, 3))
    assert pred["template_miss"].is_cuda and int(pred["template_miss"].cpu()[0]) == 0
    # class ids as a device tensor are taken as they are: the same bits, replayed or relaunched
    call2 = _cached_call(data, data["obj_idx"].cuda())
    with torch.no_grad():
        pred2 = net(call2)
    for k in ("rot_pred", "trans_pred", "conf", "F_Xo_p"):
        assert torch.equal(pred2[k], pred[k]), k
    assert torch.equal(call2["labels"]["points_tmp"].cpu(), xyz)


def test_a_device_side_miss_travels_with_the_predictions(dcl):
    """device ids are never read back: an id that is not cached raises the flag and that crop's template side is zeros"""
    n = 256
    net, _, _ = _network(dcl, n, n, graph_max_batch=0)
    data = dcl.synth.make_batch(2, n, n, first=40)
    net.cache_templates(_templates(dcl, data["obj_idx"].tolist(), n), LIMIT)
    ids = data["obj_idx"].clone()
    ids[1] = 11                                                                          # a class nobody cached
    call = _cached_call(data, ids.cuda())
    with torch.no_grad():
        pred = net(call)
    assert int(pred["template_miss"].cpu()[0]) == 1
    assert not call["labels"]["points_tmp"][1].any() and call["labels"]["points_tmp"][0].any()


# ------------------------------------------------------------------------------------------- 2. entries stand alone
def test_entries_do_not_depend_on_their_neighbours(dcl):
    n = 256
    net, _, _ = _network(dcl, n, n, graph_max_batch=0)
    tpl = _templates(dcl, (19, 20, 0), n)
    three = net.cache_templates(tpl, LIMIT)
    rows3 = three.rows[three.class_ids.index(20)].clone()
    assert rows3.abs().max() > 0
    alone = net.cache_templates({20: tpl[20]}, LIMIT)
    assert alone is net.template_cache and alone.class_ids == [20]
    assert torch.equal(alone.rows[0], rows3)
    other = net.cache_templates({20: tpl[20], 0: tpl[0]}, LIMIT)                         # ... nor on the order of the slots
    assert torch.equal(other.rows[other.class_ids.index(20)], rows3)
    assert torch.equal(rows3[:, 640:643].cpu(), tpl[20]["feats"][:, 4:7])


# ------------------------------------------------------------------------------------------- 3. the cache follows the weights
def test_cache_follows_the_weights(dcl):
    n = 256
    net, sd, _ = _network(dcl, n, n, graph_max_batch=0)
    data = dcl.synth.make_batch(3, n, n, first=40)
    tpl = _templates(dcl, data["obj_idx"].tolist(), n)
    cache = net.cache_templates(tpl, LIMIT)
    address = cache.rows.data_ptr()
    keys = ("rot_pred", "trans_pred", "conf", "F_Xo_p")
    with torch.no_grad():
        before = {k: v.clone() for k, v in net(_cached_call(data)).items()}
        w = net.backbone_tmp.module1[0].layers[0].weight
        w.mul_(1.5)                                                                      # in place: only the version counter tells
        after = net(_cached_call(data))
    assert net.template_cache is cache and cache.rows.data_ptr() == address              # recomputed into the same tensor
    fresh, _, _ = _network(dcl, n, n, sd=copy.deepcopy(net.state_dict()), graph_max_batch=0)
    fresh.cache_templates(tpl, LIMIT)
    with torch.no_grad():
        want = fresh(_cached_call(data))
    assert torch.equal(fresh.template_cache.rows, cache.rows)
    for k in keys:
        assert torch.equal(after[k], want[k]), k
    assert not torch.equal(after["F_Xo_p"], before["F_Xo_p"])
    # load_state_dict, train() / eval() and a pickled copy: the next cached call has the rows of its weights again
    net.load_state_dict(sd)
    net.train()
    net.eval()
    with torch.no_grad():
        back = net(_cached_call(data))
    for k in keys:
        assert torch.equal(back[k], before[k]), k
    twin = copy.deepcopy(net)
    assert twin.template_cache is not cache and twin.template_cache.rows is None and sorted(twin.template_cache.inputs) == sorted(tpl)
    with torch.no_grad():
        again = twin(_cached_call(data))
    for k in keys:
        assert torch.equal(again[k], before[k]), k


# ------------------------------------------------------------------------------------------- 4. routing
def test_cached_and_plain_forms_are_two_graph_entries(dcl):
    n = 256
    net, _, _ = _network(dcl, n, n)
    data = dcl.synth.make_batch(1, n, n, first=40)
    net.cache_templates(_templates(dcl, data["obj_idx"].tolist(), n), LIMIT)
    with torch.no_grad():
        plain = net(data)
        assert list(net._graphs) == [(1, n, n, 64)]
        cached = net(_cached_call(data))
        assert list(net._graphs) == [(1, n, n, 64), (1, n, n, 64, "tmp_cls")]
        net(data)
        net(_cached_call(data))
    assert len(net._graphs) == 2                                                         # both replayed, nothing recaptured
    _close(cached, plain)
    ents = {len(k): e for k, e in net._graphs.items()}
    assert "tmp" not in ents[5] and "tmp" in ents[4]                                     # no template-side staging buffers
    n_plain, n_cached = ents[4].get("nodes"), ents[5].get("nodes")
    print("graph nodes: plain %s, cached %s" % (n_plain, n_cached))
    if n_plain is not None and n_cached is not None:                                     # (where the runtime lets us ask)
        assert n_cached < n_plain


def test_recaptures_keep_the_cached_form(dcl, monkeypatch):
    """Network._select_capture may capture a new graph several times (a slow two-branch capture is tried again, the better one
    kept, the other dropped and emptied): every one of them is the cached form.  The clock is scripted so that the first capture
    looks slow, the second try better and the third good: three more captures after the first."""
    import time
    n = 256
    net, _, _ = _network(dcl, n, n)
    data = dcl.synth.make_batch(2, n, n, first=40)
    net.cache_templates(_templates(dcl, data["obj_idx"].tolist(), n), LIMIT)
    seen, real_capture, real_clock = [], net._capture, time.perf_counter
    script = [0.0, 6.0, 0.0, 0.6, 0.0, 3.0, 0.0, 0.3]              # (t0, t1) of: first capture, one-stream yardstick, two retries

    def capture(f, dev, b, S, ma, tcache=None):
        seen.append((sorted(ma), tcache))
        return real_capture(f, dev, b, S, ma, tcache)
    monkeypatch.setattr(net, "_capture", capture)
    monkeypatch.setattr(time, "perf_counter", lambda: script.pop(0) if script else real_clock())
    with torch.no_grad():
        pred = net(_cached_call(data))
    monkeypatch.undo()
    assert len(seen) == 4 and all(s == (["inp"], net.template_cache) for s in seen), seen
    ent = net._graphs[(2, n, n, 64, "tmp_cls")]
    assert [k for k, _ in ent["capture_ms"]] == ["two branches", "one stream", "two branches", "two branches"]
    plain, _, _ = _network(dcl, n, n, graph_max_batch=0)
    with torch.no_grad():
        _close(pred, plain(data))
        again = net(_cached_call(data))
    assert all(torch.equal(again[k], pred[k]) for k in ("rot_pred", "trans_pred", "conf", "F_Xo_p"))


# ------------------------------------------------------------------------------------------- 5. refusals
def test_refusals(dcl):
    n = 256
    data = dcl.synth.make_batch(2, n, n, first=40)
    tpl = _templates(dcl, data["obj_idx"].tolist(), n)
    net, sd, _ = _network(dcl, n, n, graph_max_batch=0)
    with pytest.raises(ValueError, match="cache_templates"):
        net(_cached_call(data))                                                          # no cache
    net.cache_templates(tpl, LIMIT)
    with pytest.raises(ValueError, match="class 11 "):
        net(_cached_call(data, [int(data["obj_idx"][0]), 11]))                           # a host list with an unknown class
    with pytest.raises(ValueError):
        net(_cached_call(data, [int(data["obj_idx"][0])]))                               # one id for two crops
    net.train()
    with pytest.raises(ValueError, match="eval"):
        net(_cached_call(data))
    with pytest.raises(ValueError):
        net.cache_templates(tpl, LIMIT)
    compat, _, _ = _network(dcl, n, n, sd=sd, fused=False)
    with pytest.raises(ValueError, match="fused"):
        compat.cache_templates(tpl, LIMIT)
    compat.template_cache = net.template_cache
    with pytest.raises(ValueError, match="fused"):
        compat(_cached_call(data))


# ------------------------------------------------------------------------------------------- 6. the crop builder
@pytest.mark.parametrize("routing", ["launch by launch", "default"])
def test_builder_names_the_template_side(dcl, routing):
    """CropBuilder(template_ids=True) + cache_templates(builder.templates()) against the same builder without the flag through
    the plain forward -- an existing path as the yardstick"""
    from crop_scene import make_scene
    cfg = dict(input_size=256, tmp_size=256, unit_voxel_extent=[0.006] * 3, voxel_num_limit=[64] * 3, voxelization_mode=4)
    sc = make_scene(21, n_obj=3, tmp_size=256)
    for c in sc["cad_pts"]:
        sc["cad_pts"][c] = sc["cad_pts"][c] * 0.8
    kw = {"graph_max_batch": 0} if routing == "launch by launch" else {}
    net, _, _ = _network(dcl, 256, 256, **kw)
    args = (sc["img"], sc["depth"], sc["label"], sc["rois"], sc["gt_obj"])
    plain_b = dcl.crops.CropBuilder(cfg, sc["cad_pts"], sc["cad_col"])
    ids_b = dcl.crops.CropBuilder(cfg, sc["cad_pts"], sc["cad_col"], template_ids=True)
    np.random.seed(7)
    plain = plain_b.build(*args)
    np.random.seed(7)
    named = ids_b.build(*args)
    assert "tmp" not in named and named["tmp_cls"].is_cuda and named["tmp_cls"].dtype == torch.int32
    assert named["tmp_cls"].tolist() == [int(c) for c, f in zip(sc["gt_obj"], named["all_flags"].tolist()) if f]
    assert torch.equal(named["inp"]["feats"], plain["inp"]["feats"])
    tpl = ids_b.templates()
    assert sorted(tpl) == sorted(sc["cad_pts"])
    cache = net.cache_templates(tpl, cfg["voxel_num_limit"])
    assert cache.nbytes() == len(tpl) * 256 * 644 * 4
    with torch.no_grad():
        want = net(plain)
        pred = net(named)
    _close(pred, want)
    assert torch.equal(named["labels"]["points_tmp"], plain["labels"]["points_tmp"])
    assert int(pred["template_miss"].cpu()[0]) == 0
