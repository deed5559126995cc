"""EVF_XLIF_SOFT_FUSED=1 (opt-in): XLIF / ALIF FireNets built with the cells' own default, the soft reset, are routed to the fused
engine -- host logic, no GPU.  Default off: the routing and the reason strings of tests/test_host_models.py hold."""

import pytest

from event_flow_amd.models import model as M

NEURONS = {"XLIFFireNet": {"leak_v": [-4.0, 0.1], "leak_pt": [-4.0, 0.1], "t0": [0.3, 0.0], "t1": [0.5, 0.0]},
           "ALIFFireNet": {"leak_v": [-4.0, 0.1], "leak_t": [-4.0, 0.1], "t0": [0.3, 0.0], "t1": [0.5, 0.0]}}


def cfg(neuron=None, acts=("arctanspike", "arctanspike")):
    c = {"num_bins": 2, "base_num_channels": 32, "kernel_size": 3, "encoding": "cnt", "norm_input": False, "mask_output": True,
         "activations": list(acts)}
    if neuron is not None:
        c["spiking_neuron"] = dict(neuron)
    return c


@pytest.mark.parametrize("name", ["XLIFFireNet", "ALIFFireNet"])
def test_soft_reset_firenets_are_fused_only_with_the_switch(monkeypatch, name):
    monkeypatch.setenv("EVF_PATH_NOTICE", "0")
    monkeypatch.delenv("EVF_XLIF_FUSED", raising=False)
    soft = NEURONS[name]  # (no hard_reset key: the constructors' default, False)
    build = lambda **kw: M.MODELS[name](cfg(neuron=soft, **kw))  # noqa: E731
    assert not any(c.hard_reset for c in build()._cells())
    for off in (None, "0"):  # unset or 0: today's routing and reason
        if off is None:
            monkeypatch.delenv("EVF_XLIF_SOFT_FUSED", raising=False)
        else:
            monkeypatch.setenv("EVF_XLIF_SOFT_FUSED", off)
        path, why = build().compute_path
        assert path == "general" and "soft reset" in why, (path, why)
        assert why == "XLIF / ALIF cells with the soft reset or another surrogate than arctanspike (their fused kernels: hard reset, arctan)"
        assert not build()._fused()
    monkeypatch.setenv("EVF_XLIF_SOFT_FUSED", "1")
    m = build()
    assert m.compute_path == ("fused", "") and m._fused()  # (the switch is read at call time)
    assert M.MODELS[name](cfg(neuron=dict(soft, hard_reset=True))).compute_path == ("fused", "")  # the hard reset as before
    path, why = build(acts=("superspike", "superspike")).compute_path  # another surrogate: general either way
    assert path == "general" and "surrogate" in why, (path, why)
    mixed = build()  # one reset rule per network: a hard cell among soft ones stays general, and the reason says so
    mixed.G2.hard_reset = True
    path, why = mixed.compute_path
    assert path == "general" and "mixed reset rules" in why and not mixed._fused(), (path, why)
    monkeypatch.setenv("EVF_XLIF_FUSED", "0")  # the older switch wins
    assert build().compute_path == ("general", "EVF_XLIF_FUSED=0")
    assert not build()._fused()


def test_lif_firenet_is_unaffected_by_the_switch(monkeypatch):
    monkeypatch.setenv("EVF_PATH_NOTICE", "0")
    for v in ("0", "1"):
        monkeypatch.setenv("EVF_XLIF_SOFT_FUSED", v)
        assert M.LIFFireNet(cfg()).compute_path == ("fused", "")
        soft_lif = dict(leak=[-4.0, 0.1], thresh=[0.8, 0.0], hard_reset=False)
        assert M.LIFFireNet(cfg(neuron=soft_lif)).compute_path == ("fused", "")  # (LIF cells: both reset rules, as before)
