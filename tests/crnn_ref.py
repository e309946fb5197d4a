"""torch.nn restatement of the reference's CRNN (train_physionet2.py:55-117) for the CRNN tests: built in the test, run on the
CPU (float64 where a test says so); plus the margin conditions that keep ReLU masks and pool winners decided."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class ConvBlock(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.block = nn.Sequential(nn.Conv2d(cin, cout, kernel_size=(5, 5), padding=2), nn.BatchNorm2d(cout), nn.ReLU(),
                                   nn.MaxPool2d(kernel_size=(2, 2)))

    def forward(self, x):
        return self.block(x)


class CRNN(nn.Module):
    def __init__(self, input_channels=1, num_classes=2):
        super().__init__()
        self.conv1, self.conv2, self.conv3 = ConvBlock(input_channels, 32), ConvBlock(32, 64), ConvBlock(64, 128)
        self.flatten = nn.Flatten(start_dim=2)
        self.bilstm = nn.LSTM(input_size=512, hidden_size=200, num_layers=3, batch_first=True, bidirectional=True)
        self.classifier = nn.Sequential(nn.Linear(400, 64), nn.ReLU(), nn.Dropout(0.3), nn.Linear(64, num_classes))

    def front(self, x):
        x = self.conv3(self.conv2(self.conv1(x)))
        return self.flatten(x.permute(0, 3, 1, 2))

    def forward(self, x):
        out, _ = self.bilstm(self.front(x))
        return self.classifier(out.mean(dim=1))


def focal_loss(logits, targets, alpha=1.0, gamma=2.0):
    ce = F.cross_entropy(logits, targets, reduction="none")
    return (alpha * (1 - torch.exp(-ce)) ** gamma * ce).mean()


def front_only(seed):
    """the three blocks alone (same registration order), torch default initialisation from `seed`"""
    torch.manual_seed(seed)
    m = CRNN()
    del m.bilstm, m.classifier
    return m


def margin_violations(model, x, delta=1e-4):
    """[(where, what)] for every block of `model` (float64) whose BatchNorm output has a value within delta * max|z| of zero or
    a 2x2 pool window whose two largest activations differ by less than that (equal values are a tie, which both sides
    resolve alike, not a near miss).  Nothing is excluded."""
    bad, h = [], x
    for name in ("conv1", "conv2", "conv3"):
        blk = getattr(model, name).block
        z = blk[1](blk[0](h))
        d = delta * z.abs().max()
        if (z.abs() < d).any():
            bad.append((name, "pre-activation near zero"))
        N, Cn, H, W = z.shape
        r = torch.relu(z)[:, :, :H // 2 * 2, :W // 2 * 2]
        win = r.reshape(N, Cn, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, Cn, H // 2, W // 2, 4)
        top = win.sort(-1, descending=True).values
        gap = top[..., 0] - top[..., 1]
        if ((gap > 0) & (gap < d)).any():
            bad.append((name, "pool window near tie"))
        h = blk[3](blk[2](z))
    return bad
