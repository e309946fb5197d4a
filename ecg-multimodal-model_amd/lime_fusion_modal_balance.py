"""LIME modality attribution of the fusion head (reference: lime_fusion_modal_balance.py:15-195).

Same flow and names: ``FusionClassifierWrapper`` (:15-21) and ``get_embedding_batches`` (:57-95) are the SHAP module's, the
background is the class-balanced set of fused embeddings, and every test sample's fused embedding (the ``attention_fusion``
output, :149-150 -- not the plain concatenation the SHAP script explains) is explained with ``num_features = 768`` and
``num_samples = 1000`` for class 1.  ``sum |weight|`` per modality block of ``local_exp[1]`` gives the CSV row (:161-176).
lime is not a dependency: ``ecgmm.lime_tabular`` restates it on csrc/lime.hip, and a test batch is explained in one
``explain_batch`` call instead of row by row.
"""
import os

import numpy as np
import torch

from .config import Config
from .dataset import get_dataloaders
from .hip import functional as HF
from .lime_tabular import LimeTabularExplainer
from .multimodal_paper_modal_balance import ECGMultimodalModel
from .shap_fusion_modal_balance import FusionClassifierWrapper, get_embedding_batches, modal_features

__all__ = ["FusionClassifierWrapper", "get_embedding_batches", "make_predict_fn", "modality_row", "main"]


def make_predict_fn(fusion_model):
    """the reference's predict_fn (:126-131): softmax of the wrapped classifier under no_grad, device tensor in and out"""
    def predict_fn(inputs):
        with torch.no_grad():
            return HF.softmax_rows(fusion_model(inputs))
    return predict_fn


def modality_row(local_exp, dims, label, sample_id):
    """one row of the reference's CSV (:161-176) from ``local_exp[1]`` = (feature, weight) pairs; dims = (n_img, n_signal,
    n_clinical).  Percentages of sum |weight| per block, 0 where the total is 0."""
    n_img, n_signal, n_clinical = dims
    weights = {int(f): w for f, w in local_exp}
    img = np.sum([np.abs(weights.get(i, 0)) for i in range(n_img)])
    sig = np.sum([np.abs(weights.get(i, 0)) for i in range(n_img, n_img + n_signal)])
    clin = np.sum([np.abs(weights.get(i, 0)) for i in range(n_img + n_signal, n_img + n_signal + n_clinical)])
    total = img + sig + clin
    return {"Sample_ID": sample_id,
            "Image_%": img / total * 100 if total > 0 else 0,
            "Signal_%": sig / total * 100 if total > 0 else 0,
            "Clinical_%": clin / total * 100 if total > 0 else 0,
            "Label": int(label)}


def main(config=Config, model_path=None, max_samples_per_class=50, num_samples=1000, out_csv=None, quiet=False):
    import pandas as pd
    device = torch.device(config.device)
    train_loader, _val_loader, test_loader = get_dataloaders(config)
    model = ECGMultimodalModel(config).to(device)
    if model_path:
        model.load_state_dict(torch.load(model_path, map_location=device))
    model.eval()
    fusion_model = FusionClassifierWrapper(model.fusion_classifier).to(device)
    bg_embeddings = get_embedding_batches(model, train_loader, device, max_samples_per_class).numpy()
    d = model.modal_dim
    feature_names = [f"img_{i}" for i in range(d)] + [f"sig_{i}" for i in range(d)] + [f"clin_{i}" for i in range(d)]
    explainer = LimeTabularExplainer(training_data=bg_embeddings, feature_names=feature_names,
                                     class_names=["Normal", "Abnormal"], mode="classification")
    predict_fn = make_predict_fn(fusion_model)
    results, soft_weights = [], None
    for *batch, _index in test_loader:
        images, ecg_signals, clinical, labels = (t.to(device) for t in batch)
        with torch.no_grad():
            feats = modal_features(model, images, ecg_signals, clinical)
            fused, soft_weights = model.attention_fusion(*feats)
        dims = [f.shape[1] for f in feats]
        explanations = explainer.explain_batch(fused, predict_fn, num_features=len(feature_names), num_samples=num_samples)
        for b, explanation in enumerate(explanations):
            results.append(modality_row(explanation.local_exp[1], dims, labels[b].item(), len(results) + 1))
    df = pd.DataFrame(results)
    if out_csv:
        if os.path.dirname(out_csv):
            os.makedirs(os.path.dirname(out_csv), exist_ok=True)
        df.to_csv(out_csv, index=False)
    if not quiet:
        print(df.head())
        if soft_weights is not None:
            attn = soft_weights.detach().cpu()
            print(f"Attention Weights (Softmax): Image={attn[0].item():.4f} | Signal={attn[1].item():.4f} | "
                  f"Clinical={attn[2].item():.4f}")
    return df


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="LIME ANALYSIS")
    ap.add_argument("--model_path", type=str, default=None)
    main(model_path=ap.parse_args().model_path)
