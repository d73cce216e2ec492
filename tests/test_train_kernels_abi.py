"""DCL_Net.TRAIN_KERNELS, the all-kernels training configuration named once (no GPU): its keys are exactly the train_* arguments
of Network.__init__, every value is the non-default one, and an instance built with it has a default instance's state_dict
keys.  The recorder of tests/step_replay.py is shown to have teeth here as well, on plain CPU tensors and toy Functions: a
backward that scales its incoming gradient in place trips check (a), an input changed between forward and backward check (b),
and a custom node that escapes the recorder condition (c)."""
import inspect

import pytest
import torch

import step_replay as SR


def _train_args(dcl):
    sig = inspect.signature(dcl.DCL_Net.Network.__init__)
    return {k: p.default for k, p in sig.parameters.items() if k.startswith("train_")}


def test_train_kernels_names_every_train_argument_at_a_non_default_value(dcl):
    K = dcl.DCL_Net.TRAIN_KERNELS
    defaults = _train_args(dcl)
    assert len(defaults) == 9 and set(K) == set(defaults)
    for k, v in K.items():
        assert v != defaults[k], k
    assert K["train_dense"] == "point_major" and K["train_attention"] == "fused" and K["train_heads"] == "kernels"


def test_train_kernels_constructs_with_the_default_state_dict_keys(dcl):
    cfg = dcl.synth.default_cfg(256, 256)
    net = dcl.DCL_Net.Network(cfg, mode="train", **dcl.DCL_Net.TRAIN_KERNELS)
    ref = dcl.DCL_Net.Network(cfg, mode="train")
    assert list(net.state_dict().keys()) == list(ref.state_dict().keys())
    for k, v in dcl.DCL_Net.TRAIN_KERNELS.items():
        assert getattr(net, k) == v, k
    # the constraints the constant's docstring names are the constructor's
    with pytest.raises(ValueError, match="train_attention"):
        dcl.DCL_Net.Network(cfg, mode="train", **dict(dcl.DCL_Net.TRAIN_KERNELS, train_attention="materialised"))
    with pytest.raises(ValueError, match="train_dense"):
        dcl.DCL_Net.Network(cfg, mode="train", **dict(dcl.DCL_Net.TRAIN_KERNELS, train_dense="modules"))


# ---------------------------------------------------------------------------------------------------- the recorder's teeth
class _Scale(torch.autograd.Function):
    """y = 2 x; `inplace` makes the backward scale its incoming gradient where it lies"""

    @staticmethod
    def forward(ctx, x, inplace):
        ctx.inplace = inplace
        return x * 2

    @staticmethod
    def backward(ctx, g):
        if ctx.inplace:
            return g.mul_(2), None
        return g * 2, None


class _Square(torch.autograd.Function):
    """y = x^2, x kept for the backward"""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return x * x

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return 2 * x * g


def _toy(monkeypatch):
    return SR.StepRecorder([_Scale, _Square], monkeypatch)


def test_recorder_records_and_replays_a_clean_toy_step(monkeypatch):
    rec = _toy(monkeypatch)
    x = torch.arange(6.0).view(2, 3).requires_grad_(True)
    w = x.t()                                                 # a transposed view: the replay makes it contiguous
    loss = (_Square.apply(_Scale.apply(w, False)) + _Scale.apply(w, False)).sum()
    assert rec.count_custom_nodes(loss) == 3
    loss.backward()
    rec.check_all_nodes_recorded(loss)
    assert [c.cls for c in rec.calls] == [_Scale, _Square, _Scale] and all(c.grads_in is not None for c in rec.calls)
    assert rec.counts() == {"_Scale": 2, "_Square": 1}
    for c in rec.calls:
        assert rec.replay(c) == []
    rec.calls[1].outputs[0][0, 0] += 1.0                      # a tampered record does not replay
    assert rec.replay(rec.calls[1]) != []


def test_recorder_check_a_raises_when_a_backward_scales_its_incoming_gradient_in_place(monkeypatch):
    rec = _toy(monkeypatch)
    x = torch.ones(4, requires_grad=True)
    y = _Scale.apply(x, True)
    with pytest.raises(SR.ReplayError, match=r"\(a\).*_Scale"):
        (y * 3).sum().backward()


def test_recorder_check_b_raises_when_a_saved_input_changes_before_the_backward(monkeypatch):
    rec = _toy(monkeypatch)
    x = torch.ones(4, requires_grad=True)
    buf = x * 3                                               # a non-leaf the Function saves ...
    y = _Square.apply(buf)
    buf.data.add_(1.0)                                        # ... changed behind the graph (no version bump)
    with pytest.raises(SR.ReplayError, match=r"\(b\).*_Square"):
        y.sum().backward()


def test_recorder_check_c_raises_when_a_custom_node_goes_unrecorded(monkeypatch):
    rec = _toy(monkeypatch)
    x = torch.ones(4, requires_grad=True)
    y = _Scale.apply(x, False)
    rec.calls.clear()                                         # as if the call had slipped past the recorder
    y.sum().backward()
    with pytest.raises(SR.ReplayError, match=r"\(c\)"):
        rec.check_all_nodes_recorded(y.sum())
