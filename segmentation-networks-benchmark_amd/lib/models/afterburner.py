"""Afterburner -- drop-in for the reference's ``lib.models.afterburner.Afterburner`` (lib/models/afterburner.py:8-14): a
one-class ``UNet`` over ``n_channels`` planes under the attribute ``unet`` (state_dict keys ``unet.*``), the only trainable
part of torch_train_ab.py's frozen-head setup."""
from torch import nn

from lib.models.unet import UNet


class Afterburner(nn.Module):
    def __init__(self, n_channels=1):
        super().__init__()
        self.unet = UNet(n_channels=n_channels, n_classes=1)
        self.num_classes = 1

    def set_compute_dtype(self, dtype):
        self.unet.set_compute_dtype(dtype)
        return self

    def forward(self, x):
        return self.unet(x)
