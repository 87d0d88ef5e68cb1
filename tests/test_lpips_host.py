"""CPU: the LPIPS module's checkpoint contract and loaders, and the port / weight generator against tests/golden/lpips.npz."""
import numpy as np
import pytest
import torch

import nerf_sos_amd
from nerf_sos_amd import metrics

import lpips_port as port
import lpips_weights as lw


def test_state_dict_keys_and_shapes():
    sd = nerf_sos_amd.LPIPS().state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] != []
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(lw.key_shapes())
    assert len(sd) == 17
    assert torch.equal(sd["scaling_layer.shift"].flatten(), torch.tensor(lw.SHIFT))
    assert torch.equal(sd["scaling_layer.scale"].flatten(), torch.tensor(lw.SCALE))
    assert all(float(sd[f"lin{i}.model.1.weight"].min()) >= 0 for i in range(5))
    assert nerf_sos_amd.LPIPS(net="alex") is not None


def test_load_state_dict_round_trip_and_lins_duplicates():
    state = lw.make_state("wide", 3)
    m = nerf_sos_amd.LPIPS()
    m.load_state_dict(state)
    for k, v in m.state_dict().items():
        assert torch.equal(v, state[k]), k
    dup = dict(state)
    for i in range(5):
        dup[f"lins.{i}.model.1.weight"] = state[f"lin{i}.model.1.weight"]
    m2 = nerf_sos_amd.LPIPS()
    m2.load_state_dict(dup)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, state[k]), k
    with pytest.raises(RuntimeError):
        nerf_sos_amd.LPIPS().load_state_dict({k: v for k, v in state.items() if k != "lin2.model.1.weight"})


def test_load_pretrained_from_the_two_files():
    state = lw.make_state("he", 4)
    tv = {}
    for mine, theirs in zip(lw.CONV_KEYS, ("features.0", "features.3", "features.6", "features.8", "features.10")):
        tv[theirs + ".weight"], tv[theirs + ".bias"] = state[mine + ".weight"], state[mine + ".bias"]
    tv["classifier.1.weight"], tv["classifier.1.bias"] = torch.zeros(8, 8), torch.zeros(8)      # ignored
    tv["classifier.6.weight"] = torch.zeros(4, 8)
    lin = {f"lin{i}.model.1.weight": state[f"lin{i}.model.1.weight"] for i in range(5)}
    lin.update({f"lins.{i}.model.1.weight": state[f"lin{i}.model.1.weight"] for i in range(5)})    # tolerated
    m = nerf_sos_amd.LPIPS().load_pretrained(tv, lin)
    for k, v in m.state_dict().items():
        assert torch.equal(v, state[k]), k
    with pytest.raises(KeyError):
        nerf_sos_amd.LPIPS().load_pretrained({k: v for k, v in tv.items() if k != "features.8.bias"}, lin)
    with pytest.raises(KeyError):
        nerf_sos_amd.LPIPS().load_pretrained(tv, {k: v for k, v in lin.items() if k != "lin4.model.1.weight"})


def test_vgg_is_not_implemented():
    with pytest.raises(NotImplementedError):
        nerf_sos_amd.LPIPS(net="vgg")
    with pytest.raises(NotImplementedError):
        metrics.lpips(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64), net="vgg", model=object())


def test_cpu_input_raises_no_cpu_path():
    m = nerf_sos_amd.LPIPS()
    x = torch.rand(1, 3, 64, 64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.layers(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.lpips(x[0].permute(1, 2, 0), x[0].permute(1, 2, 0), format="HWC", model=m)


def test_generated_states_match_their_sha256(golden):
    g = golden("lpips")
    for kind in lw.KINDS:
        assert lw.state_sha256(lw.make_state(kind, lw.STATE_SEEDS[kind])) == str(g[f"sha256_{kind}"]), kind


def test_port_reproduces_the_fixture(golden):
    g = golden("lpips")
    states = {k: lw.make_state(k, lw.STATE_SEEDS[k]) for k in lw.KINDS}
    for ci, (name, n, h, w, sigma, kinds) in enumerate(lw.CASES):
        a, b = lw.make_images(ci)
        assert np.array_equal(a, g[f"{name}_img0"]) and np.array_equal(b, g[f"{name}_img1"]), name
        for kind in kinds:
            v, layers, f0, f1 = port.lpips(states[kind], torch.from_numpy(a), torch.from_numpy(b), torch.float64)
            assert tuple(v.shape) == (n, 1, 1, 1) and tuple(layers.shape) == (n, 5)
            # fp64 on another BLAS / thread count reorders sums: 1e-11 of the value, five orders below the tests' bar
            np.testing.assert_allclose(v.numpy(), g[f"{name}_{kind}_value"], rtol=1e-11, atol=0)
            np.testing.assert_allclose(layers.numpy(), g[f"{name}_{kind}_layers"], rtol=1e-10, atol=1e-18)
            if kind == "sparse":
                for l in (2, 4):
                    share = max(port.zero_pixel_share(f0[l]), port.zero_pixel_share(f1[l]))
                    assert 0.0 < share < 1.0, (name, l, share)


def test_smallest_legal_size_is_31():
    state = lw.make_state("he", 5)
    x = torch.rand(1, 3, 30, 30)
    with pytest.raises(RuntimeError):
        port.lpips(state, x, x, torch.float32)
    port.lpips(state, torch.rand(1, 3, 31, 31), torch.rand(1, 3, 31, 31), torch.float32)
