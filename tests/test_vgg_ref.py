"""Reference VGG classifier head (the *_ref factory names): parameter
surface, forward shapes, the reference-checkpoint converter and the
per-replica dropout stream."""
import pytest
import torch
import torch.nn as nn

from ps_pytorch_amd.models import (build_model,
                                   convert_reference_vgg_state_dict)
from ps_pytorch_amd.models.vgg import _CFG
from ps_pytorch_amd.ops.dropout import PsDropout, PsReLU
from ps_pytorch_amd.ops.linear import PsLinear

from dist_utils import run_dist

REF_NAMES = [f'vgg{d}{v}_ref' for d in (11, 13, 16, 19)
             for v in ('', '_bn', '_plain')]

HEAD_SHAPES = {
    'classifier.1.weight': (512, 512), 'classifier.1.bias': (512,),
    'classifier.4.weight': (512, 512), 'classifier.4.bias': (512,),
    'classifier.6.weight': (10, 512), 'classifier.6.bias': (10,),
}

# parameter counts of the lean-head names (num_classes=10, in_channels=3)
LEAN_PARAMS = {
    'vgg11': 9228362, 'vgg11_bn': 9228362, 'vgg11_plain': 9225610,
    'vgg13': 9413066, 'vgg13_bn': 9413066, 'vgg13_plain': 9410122,
    'vgg16': 14724042, 'vgg16_bn': 14724042, 'vgg16_plain': 14719818,
    'vgg19': 20035018, 'vgg19_bn': 20035018, 'vgg19_plain': 20029514,
}


def _n_params(m):
    return sum(p.numel() for p in m.parameters())


@pytest.mark.parametrize('name', REF_NAMES)
def test_ref_head_surface(name):
    m = build_model(name)
    head = {k: tuple(v.shape) for k, v in m.state_dict().items()
            if k.startswith('classifier.')}
    assert head == HEAD_SHAPES
    assert len(m.classifier) == 7
    kinds = [type(e) for e in m.classifier]
    assert kinds[0] is PsDropout and kinds[3] is PsDropout
    assert kinds[1] is PsLinear and kinds[4] is PsLinear
    assert kinds[5] is PsReLU and kinds[6] is PsLinear
    assert list(m.classifier[2].parameters()) == []
    assert (m.classifier[0].salt, m.classifier[0].relu) == (0, False)
    assert (m.classifier[3].salt, m.classifier[3].relu) == (1, True)
    lean = name[:-len('_ref')]
    assert _n_params(m) == LEAN_PARAMS[lean] + 525312


@pytest.mark.parametrize('name', sorted(LEAN_PARAMS))
def test_lean_param_counts_unchanged(name):
    m = build_model(name)
    assert _n_params(m) == LEAN_PARAMS[name]
    assert isinstance(m.classifier, PsLinear)


def test_ref_name_maps_to_bn_variant():
    a = build_model('VGG11_ref').state_dict()
    b = build_model('vgg11_bn_ref').state_dict()
    assert list(a) == list(b)
    assert any(k.endswith('running_mean') for k in a)
    assert not any(k.endswith('running_mean')
                   for k in build_model('VGG11_plain_ref').state_dict())


@pytest.mark.parametrize('name', ['vgg11_ref', 'vgg16_plain_ref'])
def test_ref_forward_shape(name):
    torch.manual_seed(0)
    m = build_model(name)
    x = torch.randn(2, 3, 32, 32)
    m.train()
    assert m(x).shape == (2, 10)
    m.eval()
    with torch.no_grad():
        assert m(x).shape == (2, 10)


def test_unknown_classifier_rejected():
    from ps_pytorch_amd.models.vgg import VGG
    with pytest.raises(ValueError):
        VGG('VGG11', classifier='big')


# ---- converter ----

class _TorchVGG(nn.Module):
    """Plain-torch twin with the reference's layout: conv (with bias), bn,
    relu triples and the seven-entry nn.Dropout head."""

    def __init__(self, cfg, batch_norm, num_classes=10):
        super().__init__()
        layers, c = [], 3
        for v in cfg:
            if v == 'M':
                layers.append(nn.MaxPool2d(2, 2))
                continue
            layers.append(nn.Conv2d(c, v, 3, padding=1))
            if batch_norm:
                layers.append(nn.BatchNorm2d(v))
            layers.append(nn.ReLU(inplace=True))
            c = v
        self.features = nn.Sequential(*layers)
        self.classifier = nn.Sequential(
            nn.Dropout(), nn.Linear(512, 512), nn.ReLU(True),
            nn.Dropout(), nn.Linear(512, 512), nn.ReLU(True),
            nn.Linear(512, num_classes))

    def forward(self, x):
        x = self.features(x)
        return self.classifier(x.view(x.size(0), -1))


def _twin(batch_norm):
    g = torch.Generator().manual_seed(321)
    t = _TorchVGG(_CFG['VGG11'], batch_norm)
    with torch.no_grad():
        for m in t.modules():
            if isinstance(m, nn.Conv2d):
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.5)
            elif isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape,
                                                 generator=g) * 0.3)
                m.running_var.copy_(
                    torch.rand(m.running_var.shape, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.num_batches_tracked.fill_(7)
    return t.eval()


def test_convert_bn_checkpoint_matches_twin():
    torch.manual_seed(1)
    twin = _twin(batch_norm=True)
    sd = convert_reference_vgg_state_dict(twin.state_dict(), 'vgg11_bn_ref')
    m = build_model('vgg11_bn_ref')
    m.load_state_dict(sd, strict=True)
    m.eval()
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        want, got = twin(x), m(x)
    diff = (want - got).abs().max().item()
    print(f"converter max|diff| = {diff:.3e}, max|out| = "
          f"{want.abs().max().item():.3e}")
    # measured on CPU: max|diff| = 4.098e-08 at max|out| = 1.254e-01 (fp32;
    # folding the conv bias into running_mean reorders the adds and nothing
    # else) — allow 10x
    assert diff <= 4.1e-7, diff
    assert int(m.features[1].num_batches_tracked) == 7


def test_convert_plain_checkpoint_is_identity():
    twin = _twin(batch_norm=False)
    sd_in = twin.state_dict()
    sd = convert_reference_vgg_state_dict(sd_in, 'vgg11_plain_ref')
    assert list(sd) == list(sd_in)
    for k in sd:
        assert torch.equal(sd[k], sd_in[k]), k
    m = build_model('vgg11_plain_ref')
    m.load_state_dict(sd, strict=True)
    m.eval()
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        assert torch.allclose(twin(x), m(x), atol=1e-5, rtol=1e-5)


def test_convert_rejects_lean_names():
    with pytest.raises(ValueError):
        convert_reference_vgg_state_dict({}, 'vgg11_bn')


# ---- per-replica dropout stream ----

def _stream_role(rank, world, port):
    from ps_pytorch_amd.config import JobConfig
    from ps_pytorch_amd.parallel.transport import init_distributed
    from ps_pytorch_amd.parallel.ps import ParameterServer
    from ps_pytorch_amd.parallel.worker import DistributedWorker
    cfg = JobConfig(network='VGG11_ref', dataset='Cifar10', batch_size=4,
                    compress_grad='None', wire_dtype='fp32',
                    compute_dtype='fp32', log_interval=10 ** 9,
                    eval_freq=10 ** 9)
    env = init_distributed(backend='gloo')
    cls = ParameterServer if rank == 0 else DistributedWorker
    role = cls(cfg, rank, world, env['device'])
    role.build_model(10)
    return [m.stream for m in role.network.modules()
            if isinstance(m, PsDropout)]


def test_worker_sets_dropout_stream_to_rank():
    res = run_dist(_stream_role, world=2)
    assert res[0] == [0, 0]     # the PS leaves it alone
    assert res[1] == [1, 1]
