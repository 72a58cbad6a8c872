"""The autoencoder rows of mmvae.crossval on the MI355X, on the synthetic data of tests/test_crossval_gpu.py (RNA 40, DNA 24, 5 sites,
latent 8, 300 rows, 3 folds): cross_validate(..., ("mean", "knn", "autoencoder", "vae")) yields "ae" rows whose fold metrics are
mmvae.metrics on _predict of the fitted models, fit_ae follows BestState, training lowers the validation loss, and the name "ae"
itself is still refused."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import crossval_ref as CR  # noqa: E402
from test_crossval_gpu import A, D, S, L, N, DEV, check_fold_metrics  # noqa: E402
import trainer  # noqa: E402
from mmvae import crossval as CV  # noqa: E402
from src.config import Config  # noqa: E402
from src.models import DNA2RNAAE, RNA2DNAAE  # noqa: E402

KW = dict(epochs=2, batch_size=32, latent_dim=L, n_sites=S)


@pytest.fixture(scope="module")
def data():
    tpm, beta_v, site = trainer.synthetic_dataset(N, A, D, S, Config.RANDOM_SEED)
    return dict(a=tpm.numpy(), b=beta_v.numpy(), site=site.numpy(), fold=CV.kfold_assignments(N, 3), da=tpm.to(DEV), db=beta_v.to(DEV), dsite=site.to(DEV))


@pytest.fixture(scope="module")
def runs(data):
    preds = {}
    full = CV.cross_validate(data["db"], data["da"], data["dsite"], data["fold"], "DNA -> RNA", ("mean", "knn", "autoencoder", "vae"), (5, 10),
                             seed=42, predictions=preds, **KW)
    return dict(full=full, preds=preds)


def test_ae_rows_are_the_metrics_of_the_fitted_models(runs, data):
    results = runs["full"]
    assert [r["model"] for r in results] == ["mean", "knn", "knn", "vae", "ae"]       # the reference's order
    ae = results[-1]
    assert (ae["param_name"], ae["param_value"]) == ("epochs", 2) and list(ae["fold_metrics"]) == list(CR.KEYS)
    pred = runs["preds"][("ae", 2)]
    assert pred.shape == (N, A) and bool((pred != 0).any(dim=1).all()) and not torch.equal(pred, runs["preds"][("vae", 2)])
    check_fold_metrics(ae, data["a"], lambda f, rows: pred.cpu().numpy()[rows], data["fold"], "ae")
    # the same fold, fitted again from the same seed and predicted through _predict: the row's prediction bit for bit
    fold = data["fold"]
    rows = torch.from_numpy(np.flatnonzero(fold != 1)).to(DEV)
    test = torch.from_numpy(np.flatnonzero(fold == 1)).to(DEV)
    model, _ = CV.fit_ae("dna2rna", data["da"][rows], data["db"][rows], data["dsite"][rows].contiguous(), (A, D, S, L), epochs=2, batch_size=32, seed=42, fold=1)
    assert isinstance(model, DNA2RNAAE) and not model.training
    again = CV._predict("dna2rna", model, data["db"][test], data["dsite"][test].contiguous())
    assert torch.equal(again.view(torch.int32), pred[test].view(torch.int32)), "the same seed and fold must give the same model"


def test_compare_has_the_two_ae_pairs(runs):
    pytest.importorskip("scipy.stats")
    from scipy import stats
    for metric in ("Mean R2", "MSE", "Pearson"):
        (e,) = CV.compare(runs["full"], metric)
        ae, vae = runs["full"][-1], runs["full"][-2]
        want = stats.ttest_rel(ae["fold_metrics"][metric], vae["fold_metrics"][metric])
        assert e["best_ae"] == 2 and e["ae_vs_vae"]["df"] == 2 and e["ae_vs_vae"]["t"] == pytest.approx(float(want.statistic), rel=1e-9)
        assert e["ae_vs_vae"]["p"] == pytest.approx(float(want.pvalue), rel=1e-9) and e["ae_vs_knn"]["b"] == "kNN"
        without = CV.compare([r for r in runs["full"] if r["model"] != "ae"], metric)[0]
        assert {k: v for k, v in e.items() if k in without} == without


@pytest.mark.parametrize("eager", [False, True])
@pytest.mark.parametrize("kind", ["dna2rna", "rna2dna"])
def test_fit_ae_restores_the_best_epochs_state(kind, eager, data):
    """the validation losses are stubbed as 3, 1, 2: the state after the second epoch must come back, not the last one"""
    seen = []

    def val_loss(model, epoch):
        seen.append({k: v.detach().clone() for k, v in model.state_dict().items()})
        return [3.0, 1.0, 2.0][epoch]

    model, best = CV.fit_ae(kind, data["da"][:200], data["db"][:200], data["dsite"][:200], (A, D, S, L), epochs=3, batch_size=32, eager=eager, val_loss_fn=val_loss)
    assert isinstance(model, DNA2RNAAE if kind == "dna2rna" else RNA2DNAAE)
    assert len(seen) == 3 and best.best_epoch == 1 and best.best == 1.0 and best.trigger == 1 and not model.training
    now = model.state_dict()
    assert all(torch.equal(now[k], seen[1][k]) for k in now)
    assert any(not torch.equal(seen[2][k], seen[1][k]) for k in now), "the third epoch must have moved the weights"


EPOCHS = 30


def _structured_dna(data):
    """A DNA target with learnable structure, built here because trainer.synthetic_dataset's is uniform noise independent of RNA and
    site (the expected held-out sum-BCE of any predictor is then at least the constant 0.5's, which an untrained model already is, so
    no correct training can lower it): beta_ij = sigmoid(c_j + (standardised RNA_i . r_j) / sqrt(A)), column offsets c_j ~ N(0, 1.5^2)
    and fixed directions r_j.  The offsets alone are a held-out gain: the decoder's output bias moves towards c_j on every row alike."""
    g = torch.Generator().manual_seed(7)
    a = data["da"].cpu()
    std = (a - a.mean(0)) / a.std(0)
    c, r = 1.5 * torch.randn(D, generator=g), torch.randn(A, D, generator=g)
    return torch.sigmoid(c + std @ r / A ** 0.5).to(DEV).contiguous()


@pytest.mark.parametrize("kind", ["dna2rna", "rna2dna"])
def test_training_lowers_the_validation_loss(kind, data):
    """A trained fold's BEST validation loss (BestState.best over the epochs) is below the untrained model's on the same held-out rows
    (the same seed: the same initialisation).  No margin.  DNA -> RNA on the synthetic data as it is (the RNA target has a column mean
    near 1 to learn); RNA -> DNA on the same RNA with the structured target of _structured_dna.  The epochs are chosen by reasoning, not
    from a result: an epoch is 7 steps of 32 rows, Adam moves a parameter by at most the learning rate (5e-4) per step, and the
    BatchNorm running statistics the eval-mode pass reads are a 0.9-per-step moving average (48 % still initial after one epoch); 30
    epochs are 210 steps, a tenth of a unit for every bias."""
    rna, dna, site = data["da"], (data["db"] if kind == "dna2rna" else _structured_dna(data)), data["dsite"]

    def held_out_loss(model):
        with torch.no_grad():
            return CV._ae_forward_loss(kind, model, rna[250:], dna[250:], site[250:]).item()

    model, best = CV.fit_ae(kind, rna[:250], dna[:250], site[:250], (A, D, S, L), epochs=EPOCHS, batch_size=32,
                            val_loss_fn=lambda model, epoch: held_out_loss(model))
    torch.manual_seed((42 * 1000 + 0) * 100003)                       # fit_ae's seed for (seed 42, fold 0)
    untrained = held_out_loss((DNA2RNAAE if kind == "dna2rna" else RNA2DNAAE)(A, D, S, L).to(DEV).eval())
    print(f"fit_ae {kind}: held-out loss untrained {untrained:.4f}, best of {EPOCHS} epochs {best.best:.4f} (epoch {best.best_epoch})")
    assert np.isfinite(best.best) and best.best < untrained


def test_the_name_ae_is_still_refused(data):
    with pytest.raises(ValueError):
        CV.cross_validate(data["db"], data["da"], data["dsite"], data["fold"], "DNA -> RNA", ("ae",))
    with pytest.raises(ValueError):
        CV.cross_validate(data["db"], data["da"], data["dsite"], data["fold"], "DNA -> RNA", ("mean", "ae", "autoencoder"))
