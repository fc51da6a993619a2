"""PixelWeightLayer of DiscoNet's fusion (reference: opencood/models/fuse_modules/disco_fuse.py, imported by
fusion_in_one.py:156; the layer comes from the DiscoNet / CoAlign lineage): one logit per pixel from a four-layer 1x1 MLP over
cat(warped neighbour, ego), 2C -> 128 -> 32 -> 8 -> 1.  Plain torch layers: this is the CPU, gradient and training arithmetic;
inference on the device folds the BatchNorms and runs inside heal_disco_fuse (fusion_in_one.DiscoFusion)."""
import torch.nn as nn
import torch.nn.functional as F


class PixelWeightLayer(nn.Module):
    def __init__(self, channel):
        super().__init__()
        self.conv1_1 = nn.Conv2d(channel * 2, 128, kernel_size=1, stride=1, padding=0)
        self.bn1_1 = nn.BatchNorm2d(128)
        self.conv1_2 = nn.Conv2d(128, 32, kernel_size=1, stride=1, padding=0)
        self.bn1_2 = nn.BatchNorm2d(32)
        self.conv1_3 = nn.Conv2d(32, 8, kernel_size=1, stride=1, padding=0)
        self.bn1_3 = nn.BatchNorm2d(8)
        self.conv1_4 = nn.Conv2d(8, 1, kernel_size=1, stride=1, padding=0)

    def forward(self, x):
        x = x.view(-1, x.size(-3), x.size(-2), x.size(-1))
        x_1 = F.relu(self.bn1_1(self.conv1_1(x)))
        x_1 = F.relu(self.bn1_2(self.conv1_2(x_1)))
        x_1 = F.relu(self.bn1_3(self.conv1_3(x_1)))
        x_1 = F.relu(self.conv1_4(x_1))
        return x_1
