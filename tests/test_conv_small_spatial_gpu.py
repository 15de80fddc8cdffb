"""3x3 stride-1 pad-1 wgrad at 2x2 and 1x1 spatial size (VGG's last conv
stage is 2x2 on CIFAR inputs). These shapes used to take the row-halo wgrad
kernel, whose LDS halo image holds 48 pixels per step while Q = 2 stages 64:
dw came out wrong and differed from run to run, which is what made eager
and hipGraph VGG training drift apart."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('hw', [2, 1])
@pytest.mark.parametrize('C,K', [(64, 64), (128, 192)])
def test_wgrad_small_spatial(hw, C, K):
    from ps_pytorch_amd.ops.conv import PsConv2d
    g = torch.Generator().manual_seed(5)
    x = torch.randn(64, C, hw, hw, generator=g).bfloat16().cuda()
    x = x.contiguous(memory_format=torch.channels_last)
    dy = torch.randn(64, K, hw, hw, generator=g).bfloat16().cuda()
    dy = dy.contiguous(memory_format=torch.channels_last)
    conv = PsConv2d(C, K, 3, padding=1, bias=False).cuda().bfloat16()
    conv = conv.to(memory_format=torch.channels_last)

    def dw():
        conv.weight.grad = None
        conv(x).backward(dy)
        return conv.weight.grad.clone()

    first = dw()
    for _ in range(3):
        assert torch.equal(dw(), first)     # no run-to-run difference
    w32 = conv.weight.detach().float().requires_grad_(True)
    F.conv2d(x.float(), w32, padding=1).backward(dy.float())
    ref = w32.grad
    # bf16 output: RNE relative error 2^-9 (allow 2^-8); fp32 accumulation
    # over <= 256 products in a different order: far below 1e-3 of the scale
    err = (first.float() - ref).abs()
    bound = ref.abs() * 2.0 ** -8 + 1e-3 * ref.abs().max()
    print(f"hw={hw} C={C} K={K}: max err {err.max().item():.3e}, "
          f"max|ref| {ref.abs().max().item():.3e}")
    assert (err <= bound).all(), (err.max().item(), ref.abs().max().item())
