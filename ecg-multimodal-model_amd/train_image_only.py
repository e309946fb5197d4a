"""Image-only ResNet18 classifier and its training loop (reference: train_image_only.py:92-310;
BASELINE config 2).  ``ImageOnlyClassifier`` keeps the ``image_encoder.*`` state_dict prefix.  The loop itself (last.pth
every epoch, best.pth on a lower validation loss, stop after ``Config.patience`` misses) is ``ecgmm.training.fit``."""
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, Dataset

from . import training as T
from .config import Config
from .hip import functional as HF
from .hip import nn as hnn
from .image_encoder import resnet18
from .optim import FusedAdam


class ImageOnlyClassifier(nn.Module):
    def __init__(self, compute_dtype=None, pretrained_state_dict=None):
        super().__init__()
        cd = compute_dtype or getattr(Config, "compute_dtype", "bf16")
        # the reference fetches IMAGENET1K_V1 weights here (:95) -- offline: random init, or a local state_dict
        self.image_encoder = resnet18(compute_dtype=cd)
        if pretrained_state_dict is not None:
            self.image_encoder.load_state_dict(pretrained_state_dict, strict=False)
        self.image_encoder.fc = hnn.Linear(self.image_encoder.fc.in_features, Config.num_classes)

    def forward(self, x):
        return self.image_encoder(x)


class ImageOnlyDataset(Dataset):
    """Synthetic stand-in for train_image_only.py:20-41 (image, label)."""

    def __init__(self, size, seed=0):
        self.size, self.seed = size, seed

    def __len__(self):
        return self.size

    def __getitem__(self, idx):
        g = torch.Generator().manual_seed(self.seed * 1000003 + idx)
        label = torch.randint(0, Config.num_classes, (), generator=g)
        img = torch.randn(3, Config.img_height, Config.img_width, generator=g).clamp_(-1, 1)
        img[0, : Config.img_height // 4] += 0.3 * float(label)
        return img.clamp_(-1, 1), label.to(torch.long)


def get_imageonly_dataloaders():
    mk = lambda n, s, sh: DataLoader(ImageOnlyDataset(n, s), batch_size=Config.batch_size, shuffle=sh, drop_last=sh)
    return (mk(getattr(Config, "synthetic_train_size", 256), Config.seed, True),
            mk(getattr(Config, "synthetic_val_size", 32), Config.seed + 1, False),
            mk(getattr(Config, "synthetic_test_size", 32), Config.seed + 2, False))


def main(num_epochs=None, quiet=False):
    """-> ([(train loss, train accuracy, val loss, val accuracy) per epoch], checkpoint directory)"""
    T.seed_all(Config.seed)
    device = torch.device(Config.device)
    train_loader, val_loader, test_loader = get_imageonly_dataloaders()
    model = ImageOnlyClassifier().to(device)
    optimizer = FusedAdam(model.parameters(), lr=Config.lr)          # :111
    ckpt_dir = T.run_dir(Config.checkpoint_dir)

    def step(batch):
        images, labels = batch[0].to(device), batch[1].to(device)
        out = model(images)
        return HF.cross_entropy(out, labels), out, labels             # nn.CrossEntropyLoss(), :110

    def train_pass():
        model.train()
        return T.run_epoch(train_loader, step, optimizer)

    def val_pass():
        model.eval()
        return T.run_epoch(val_loader, step)

    def on_epoch(h, _extras):
        if not quiet:
            print(f"epoch {h['epoch']}: train {h['train_loss']:.4f}/{h['train_acc']:.3f} "
                  f"val {h['val_loss']:.4f}/{h['val_acc']:.3f}")

    history = T.fit(model, optimizer, train_pass, val_pass, ckpt_dir, num_epochs or Config.num_epochs,
                    patience=Config.patience, on_epoch=on_epoch)
    return [(h["train_loss"], h["train_acc"], h["val_loss"], h["val_acc"]) for h in history], ckpt_dir


if __name__ == "__main__":
    main()
