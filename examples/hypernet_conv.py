"""
A hypernetwork in the HyperMorph style on MI355X: a small dense network maps one scalar hyper-parameter per batch entry to the kernels
and biases of two `HyperConv3DFromDense` layers, which then convolve that entry's image with ITS OWN weights.

    python examples/hypernet_conv.py --steps 3

Every batch entry carries a different hyper-parameter, so every entry is convolved with different kernels -- in one launch per layer
(`nrt_hyperconv3d_f32`).  The backward gives the per-entry kernel gradients (`nrt_hyperconv3d_wgrad_f32`), which torch carries on into
the dense maps inside the layers and into the hypernetwork in front of them.
"""

import argparse
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import neurite_amd as ne  # noqa: E402


class HyperNet(nn.Module):
    def __init__(self, features=16, hidden=32):
        super().__init__()
        self.hyper = nn.Sequential(nn.Linear(1, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU())
        self.conv0 = ne.layers.HyperConv3DFromDense(features, 3, padding='same', activation='elu')
        self.conv1 = ne.layers.HyperConv3DFromDense(1, 3, padding='same')

    def forward(self, image, lam):
        h = self.hyper(lam)                                   # [B, hidden]: the last hypernetwork layer
        return self.conv1([self.conv0([image, h]), h])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--size', type=int, default=32)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--lr', type=float, default=1e-3)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = HyperNet().to(dev)
    image = torch.randn(args.batch, args.size, args.size, args.size, 1, device=dev)
    lam = torch.rand(args.batch, 1, device=dev)
    # a target that depends on the hyper-parameter: the image scaled by it
    target = image * lam.reshape(-1, 1, 1, 1, 1)
    net(image, lam)                                           # the FromDense layers create their parameters on the first call
    opt = torch.optim.SGD(net.parameters(), lr=args.lr)
    for step in range(args.steps):
        opt.zero_grad()
        loss = ((net(image, lam) - target) ** 2).mean()
        loss.backward()
        opt.step()
        print(json.dumps({'step': step, 'loss': float(loss.detach())}))
    names = sorted(n for n, _ in net.conv0.named_parameters())
    print(json.dumps({'conv0_parameters': names, 'grad_norm_hypernet_first_layer': float(net.hyper[0].weight.grad.norm())}))


if __name__ == '__main__':
    main()
