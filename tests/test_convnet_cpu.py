"""CPU: what I3D, Inception V3 and LPIPS hand to the shared conv (omnitokenizer_amd/convnet.py): the packed weights of a
synthetic state_dict of each, bit for bit.  The digests pin fold_bn (its fp64 expression and its order), the order in which
the fused 1x1 siblings are concatenated, pack_conv_weight and the mapping from state_dict keys to packed entries."""
import hashlib

import pytest
import torch

from omnitokenizer_amd import _lib, i3d, inception, lpips, synth


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import build
    build.build()
    return _lib.load()


def _update(h, obj):
    if isinstance(obj, torch.Tensor):
        h.update(f"{obj.dtype}{tuple(obj.shape)}".encode())
        h.update(obj.contiguous().numpy().tobytes())
    elif isinstance(obj, dict):
        for k in sorted(obj):
            h.update(k.encode())
            _update(h, obj[k])
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _update(h, v)
    else:
        h.update(repr(obj).encode())


def packed_digest(model) -> str:
    """sha256 over every packed tensor of model._weights(cpu), in key order (LPIPS: convs, lins, scale, shift)"""
    h = hashlib.sha256()
    _update(h, model._weights(torch.device("cpu")))
    return h.hexdigest()


NETWORKS = {
    "i3d": (lambda: i3d.InceptionI3d(400), lambda: synth.synth_i3d_state_dict(2)),
    "inception": (lambda: inception.InceptionV3([3]), lambda: synth.synth_fid_inception_state_dict(2)),
    "lpips": (lambda: lpips.LPIPS(), lambda: synth.synth_lpips_state_dict(2)),
}
# recorded with the commit before omnitokenizer_amd/convnet.py
PACKED_DIGESTS = {
    "i3d": "27f5baa3612558831d6949fe74dfead3133ea1563b687b27ff17251e234d165d",
    "inception": "e8ef7a2c5078b7335d8ce0ab0f0584356707ce6e54b3b56e04ecf155d901cae1",
    "lpips": "48c739a661a7860512855bec74b17eb966ce374b99068cb4afebabc67c5c2254",
}


@pytest.mark.parametrize("net", list(NETWORKS))
def test_packed_weights_bit_for_bit(lib, net):
    make, sd = NETWORKS[net]
    m = make()
    m.load_state_dict(sd())
    assert packed_digest(m) == PACKED_DIGESTS[net]
    assert m._weights(torch.device("cpu")) is m._weights(torch.device("cpu"))   # packed once per device
    m.load_state_dict(sd())
    assert packed_digest(m) == PACKED_DIGESTS[net]                               # and again after a reload
