"""12-lead signal-only trainer (reference: train_signal_12_af.py:238-444; BASELINE config 5):
ResNet1D_SE(input_channels=12) + FocalLoss(1, 2) + Adam(1e-3) + OneCycleLR(max_lr=1e-3) stepped per
batch; last.pth every epoch, best.pth on a lower validation loss, stop after 5 misses (``ecgmm.training.fit``).
Data: synthetic [12, L] series (the reference's per-patient xlsx files are private)."""
import torch
from torch.utils.data import DataLoader, Dataset

from . import training as T
from .config import Config
from .optim import FusedAdam
from .signal_model import FocalLoss, ResNet1D_SE


class SignalOnlyDataset(Dataset):
    def __init__(self, size, leads=12, length=5000, seed=0):
        self.size, self.leads, self.length, self.seed = size, leads, length, seed

    def __len__(self):
        return self.size

    def __getitem__(self, idx):
        g = torch.Generator().manual_seed(self.seed * 1000003 + idx)
        label = torch.randint(0, 2, (), generator=g)
        x = torch.randn(self.leads, self.length, generator=g)
        t = torch.arange(self.length, dtype=torch.float32)
        x = x + 0.5 * float(label) * torch.sin(t * (2 * 3.14159265 / 200.0))
        return x, label.to(torch.long)


def get_signalonly_dataloaders(batch_size=8, length=5000):
    mk = lambda n, s, sh: DataLoader(SignalOnlyDataset(n, 12, length, s), batch_size=batch_size, shuffle=sh,
                                     drop_last=sh)
    return mk(128, 42, True), mk(32, 43, False), mk(32, 44, False)


def main(epochs=30, batch_size=8, length=5000, quiet=False):
    """-> ([(train loss, train accuracy, val loss, val accuracy) per epoch], checkpoint directory)"""
    T.seed_all(42)
    device = torch.device(Config.device)
    train_loader, val_loader, test_loader = get_signalonly_dataloaders(batch_size, length)
    model = ResNet1D_SE(input_channels=12, compute_dtype=getattr(Config, "compute_dtype", "bf16")).to(device)
    criterion = FocalLoss(alpha=1.0, gamma=2.0)
    optimizer = FusedAdam(model.parameters(), lr=0.001)
    scheduler = torch.optim.lr_scheduler.OneCycleLR(optimizer, max_lr=0.001, steps_per_epoch=len(train_loader),
                                                    epochs=epochs)
    ckpt_dir = T.run_dir("./checkpoints")

    def step(batch):
        signals, labels = batch[0].to(device), batch[1].to(device)
        out = model(signals)
        return criterion(out, labels), out, labels

    def train_pass():
        model.train()
        return T.run_epoch(train_loader, step, optimizer, scheduler)

    def val_pass():   # the accuracy is accumulated over the batches (the reference's `=` at :295 is a bug)
        model.eval()
        return T.run_epoch(val_loader, step)

    def on_epoch(h, _extras):
        if not quiet:
            print(f"epoch {h['epoch']}: train {h['train_loss']:.4f}/{h['train_acc']:.3f} "
                  f"val {h['val_loss']:.4f}/{h['val_acc']:.3f}")

    history = T.fit(model, optimizer, train_pass, val_pass, ckpt_dir, epochs, patience=5, on_epoch=on_epoch)
    return [(h["train_loss"], h["train_acc"], h["val_loss"], h["val_acc"]) for h in history], ckpt_dir


if __name__ == "__main__":
    main()
