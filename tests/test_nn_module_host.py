"""func_VAENN_MQAM.Net / Net_BN without a GPU: import, construction on the CPU, the reference's state_dict, its initialisation bounds, the
converters to and from the engine's flat vectors, the refusal of CPU inputs and the size functions of the encoder ABI."""
import numpy as np
import pytest
import torch

import _ref_vaenn as ref

NET_KEYS = ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]
BN_KEYS = NET_KEYS + ["batch1.weight", "batch1.bias", "batch1.running_mean", "batch1.running_var", "batch1.num_batches_tracked"]
SHAPES = [(25, 3, 8, 2), (11, 5, 4, 3), (63, 9, 2, 1), (1, 1, 8, 8)]


def _classes():
    from vae_equalizer_amd.func_VAENN_MQAM import Net, Net_BN
    return Net, Net_BN


def test_classes_import_and_are_listed():
    import vae_equalizer_amd
    Net, Net_BN = _classes()
    assert issubclass(Net, torch.nn.Module) and issubclass(Net_BN, torch.nn.Module)
    assert {"Net", "Net_BN", "nn_encode", "net_to_theta", "theta_to_net"} <= set(vae_equalizer_amd.__all__)
    assert vae_equalizer_amd.Net is Net and vae_equalizer_amd.Net_BN is Net_BN


@pytest.mark.parametrize("k1,k2,n,sps", SHAPES)
def test_state_dict_equals_the_reference(k1, k2, n, sps):
    Net, Net_BN = _classes()
    C_ = 2 * n
    shapes = {"fc1.weight": (C_, 2, k1), "fc1.bias": (C_,), "fc2.weight": (C_, C_, k2), "fc2.bias": (C_,), "batch1.weight": (C_,),
              "batch1.bias": (C_,), "batch1.running_mean": (C_,), "batch1.running_var": (C_,), "batch1.num_batches_tracked": ()}
    for cls, keys in ((Net, NET_KEYS), (Net_BN, BN_KEYS)):
        net = cls(k1, k2, n, sps)
        sd = net.state_dict()
        assert list(sd.keys()) == keys
        for k in keys:
            assert tuple(sd[k].shape) == shapes[k], k
            assert sd[k].dtype == (torch.int64 if k.endswith("num_batches_tracked") else torch.float32), k
        assert [nm for nm, _ in net.named_parameters()] == [k for k in keys if "running" not in k and "tracked" not in k]
        assert (net.fc1.padding, net.fc2.padding, net.fc2.stride) == ((k1 // 2,), (k2 // 2,), (sps,))
        net.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)


@pytest.mark.parametrize("k1,k2,n,sps", SHAPES)
def test_initialisation_bounds(k1, k2, n, sps):
    """xavier_uniform_: |w| <= sqrt(6 / (fan_in + fan_out)); kaiming_uniform_ (a = 0): |w| <= sqrt(6 / fan_in); PyTorch's default bias
    bound 1 / sqrt(fan_in); BatchNorm starts at (1, 0) with running statistics (0, 1)."""
    Net, Net_BN = _classes()
    C_ = 2 * n
    torch.manual_seed(k1 + n)
    for cls in (Net, Net_BN):
        net = cls(k1, k2, n, sps)
        b1 = (6.0 / (2 * k1)) ** 0.5 if cls is Net_BN else (6.0 / (2 * k1 + C_ * k1)) ** 0.5
        b2 = (6.0 / (2 * C_ * k2)) ** 0.5
        assert net.fc1.weight.abs().max() <= b1 and net.fc2.weight.abs().max() <= b2
        assert net.fc1.weight.abs().max() > 0.5 * b1 and net.fc2.weight.abs().max() > 0.5 * b2
        assert net.fc1.bias.abs().max() <= (2 * k1) ** -0.5 and net.fc2.bias.abs().max() <= (C_ * k2) ** -0.5
        if cls is Net_BN:
            b = net.batch1
            assert torch.all(b.weight == 1) and torch.all(b.bias == 0) and torch.all(b.running_mean == 0) and torch.all(b.running_var == 1)
            assert int(b.num_batches_tracked) == 0


@pytest.mark.parametrize("bn", [False, True])
@pytest.mark.parametrize("k1,k2,n,sps", SHAPES[:3])
def test_theta_round_trip_matches_engine_offsets(k1, k2, n, sps, bn):
    from vae_equalizer_amd.engine import NNEngine
    from vae_equalizer_amd.func_VAENN_MQAM import net_to_theta, theta_to_net
    Net, Net_BN = _classes()
    M = 13
    o = NNEngine.offsets(type("E", (), dict(n_lev=n, k1=k1, k2=k2, M=M, batch_norm=bn))())
    assert o == ref.offsets(n, k1, k2, M, bn)
    rng = np.random.default_rng(3)
    theta = torch.from_numpy(ref.init_theta(rng, n, k1, k2, M, bn))
    bnv = torch.from_numpy(ref.random_bn(rng, n)) if bn else None
    net = (Net_BN if bn else Net)(k1, k2, n, sps)
    h = theta_to_net(theta, net, bnv)
    assert tuple(h.shape) == (2, M) and torch.equal(h.reshape(-1), theta[o[-2]:])
    for p, a, b in zip(net._params(), o[:-1], o[1:]):
        assert torch.equal(p.detach().reshape(-1), theta[a:b])
    t2, b2 = net_to_theta(net, h)
    assert torch.equal(t2, theta) and t2.numel() == o[-1]
    assert (b2 is None) if not bn else torch.equal(b2, bnv)
    with pytest.raises(ValueError):
        theta_to_net(theta[:o[-2]], net)


def test_cpu_input_is_refused():
    from vae_equalizer_amd import _native as nat
    Net, Net_BN = _classes()
    for cls in (Net, Net_BN):
        with pytest.raises(nat.VaeqError, match="device tensors"):
            cls(5, 3, 4, 2)(torch.zeros(1, 2, 40))
    with pytest.raises(ValueError):
        Net(5, 3, 4, 2)(torch.zeros(2, 40))


def test_size_functions():
    from vae_equalizer_amd import _native as nat
    L = nat.lib()
    for n in (2, 4, 8):
        for k1, k2, M in ((25, 3, 25), (1, 1, 1), (63, 9, 63)):
            for bn in (0, 1):
                assert L.vaeq_nn_enc_param_count(n, k1, k2, bn) == L.vaeq_nn_param_count(M, n, k1, k2, bn) - 2 * M
                assert L.vaeq_nn_enc_param_count(n, k1, k2, bn) == ref.offsets(n, k1, k2, M, bool(bn))[-2]
                a, b = L.vaeq_nn_enc_lds_bytes(600, 2, n, k1, k2, bn), L.vaeq_nn_enc_lds_bytes(1200, 2, n, k1, k2, bn)
                assert 0 < a < b
    assert L.vaeq_nn_enc_lds_bytes(600, 2, 8, 25, 3, 1) >= L.vaeq_nn_enc_lds_bytes(600, 2, 8, 25, 3, 0)
    for args in ((3, 25, 3, 0), (8, 65, 3, 0), (8, 24, 3, 0), (8, 25, 11, 1), (8, 25, 2, 1), (8, 0, 3, 0)):
        assert L.vaeq_nn_enc_param_count(*args) == -2, args
    for args in ((0, 2, 8, 25, 3, 0), (600, 0, 8, 25, 3, 0), (600, 9, 8, 25, 3, 0), (600, 2, 3, 25, 3, 0), (600, 2, 8, 65, 3, 0), (-5, 2, 8, 25, 3, 1)):
        assert L.vaeq_nn_enc_lds_bytes(*args) == -2, args
