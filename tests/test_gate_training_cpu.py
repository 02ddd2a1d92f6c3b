"""Opt-in training of the MoE gate, without a GPU: the `train_gate` config field, what unfreezing and freezing do to the gate with
and without it, in both MoE modalities."""
import warnings

import pytest
import torch

from tests.test_gating_cpu import _modality, _write_gate


def _build(tmp_path, pep, **cfg):
    _write_gate(tmp_path / "gate")
    m, _ = _modality(tmp_path, str(tmp_path / "gate"), pep)
    for k, v in cfg.items():
        setattr(m.config, k, v)
    return m


@pytest.mark.parametrize("pep", [False, True])
def test_config_field(pep):
    from multimeditron_amd.model.modalities import MOEImageConfig, MOEImageConfigPEP
    cls = MOEImageConfigPEP if pep else MOEImageConfig
    assert "train_gate" not in cls().to_dict() and cls().train_gate is False
    assert "train_gate" not in cls(train_gate=False).to_dict()
    d = cls(train_gate=True).to_dict()
    assert d["train_gate"] is True
    assert cls.from_dict(d).train_gate is True and cls.from_dict(cls().to_dict()).train_gate is False


@pytest.mark.parametrize("pep", [False, True])
def test_unfreeze_trains_the_gate(tmp_path, pep):
    m = _build(tmp_path, pep, train_gate=True)
    gate = m.gating_network
    assert len(list(gate.parameters())) == 161
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # no warning may be emitted
        m.train()
        assert not gate.training and not any(p.requires_grad for p in gate.parameters())      # not before the unfreeze
        m.unfreeze_modality_embedder()
        assert all(p.requires_grad for p in gate.parameters())
        assert all(mod.training for mod in gate.modules())
        m.eval()
        assert not any(mod.training for mod in gate.modules())
        m.train()
        assert all(mod.training for mod in gate.modules())
        m.freeze_modality_embedder()
        assert not any(p.requires_grad for p in gate.parameters()) and not any(mod.training for mod in gate.modules())
        m.train()
        assert not gate.training
        m.unfreeze_all()
        assert all(p.requires_grad for p in gate.parameters()) and all(mod.training for mod in gate.modules())


@pytest.mark.parametrize("pep", [False, True])
@pytest.mark.parametrize("explicit", [False, True], ids=["key-absent", "train_gate-false"])
def test_default_stays_frozen(tmp_path, pep, explicit, monkeypatch):
    """the assertions of tests/test_gating_cpu.py::test_gate_stays_frozen, with the key absent and with train_gate=False"""
    from multimeditron_amd.model.modalities.image_modality_moe import _FrozenGate
    monkeypatch.setattr(_FrozenGate, "_warned_frozen_gate", True)       # the once-per-process warning is left for the tests that pin it
    m = _build(tmp_path, pep, **({"train_gate": False} if explicit else {}))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.train()
        m.unfreeze_modality_embedder()
        assert not any(p.requires_grad for p in m.gating_network.parameters())
        assert not m.gating_network.training and not any(mod.training for mod in m.gating_network.modules())
        assert all(p.requires_grad for p in m.experts.parameters()) and m.training
        m.unfreeze_all()
        assert not any(p.requires_grad for p in m.gating_network.parameters())
        m.freeze_modality_embedder()
        m.train()
        assert not m.gating_network.training
    assert "train_gate" not in type(m.config)().to_dict()


def test_gate_alone_train_is_a_no_op_until_trainable():
    from multimeditron_amd.model.modalities.gating import GatingNetwork, GatingNetworkConfig
    g = GatingNetwork(GatingNetworkConfig(num_classes=3))
    assert not g.train().training
    g.set_trainable(True)
    assert not g.training and all(p.requires_grad for p in g.parameters())
    assert g.train().training and all(mod.training for mod in g.modules())
    g.set_trainable(False)
    assert not g.training and not any(mod.training for mod in g.modules()) and not any(p.requires_grad for p in g.parameters())


@pytest.mark.parametrize("pep", [False, True])
def test_a_callable_plug_is_left_alone(tmp_path, pep):
    fn = lambda px: None
    m, _ = _modality(tmp_path, "stub", pep, gating_network=fn)
    m.config.train_gate = True
    m.train()
    m.unfreeze_modality_embedder()
    m.freeze_modality_embedder()
    assert m.gating_network is fn
