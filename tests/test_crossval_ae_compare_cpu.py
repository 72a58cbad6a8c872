"""crossval.compare() with AE rows: on hand-made result dicts the two new pairs ae_vs_vae and ae_vs_knn equal scipy.stats.ttest_rel
(t, p, df) on the best AE (by mean_Mean R2) against the best VAE / the best kNN; results without AE rows give exactly the dict the
comparison gave before the AE rows existed (restated here from the keys it had)."""
import numpy as np
import pytest

from mmvae import crossval as CV


def _row(direction, model, pname, pvalue, rng, level):
    scores = {k: list(level + 0.05 * rng.standard_normal(7)) for k in CV.METRIC_KEYS}
    return CV.aggregate(direction, model, pname, pvalue, 1.0, scores)


def _results(with_ae, seed=0):
    rng, rng_ae = np.random.default_rng(seed), np.random.default_rng(seed + 1)          # the AE rows leave the other rows as they are
    out = []
    for direction in ("DNA -> RNA", "RNA -> DNA"):
        out += [_row(direction, "mean", "dummy", 0, rng, 0.1), _row(direction, "knn", "k", 5, rng, 0.5), _row(direction, "knn", "k", 10, rng, 0.55),
                _row(direction, "knn_site", "k", 5, rng, 0.52), _row(direction, "vae", "epochs", 3, rng, 0.6)]
        if with_ae:
            out += [_row(direction, "ae", "epochs", 3, rng_ae, 0.58), _row(direction, "ae", "epochs", 5, rng_ae, 0.62)]
    return out


@pytest.mark.parametrize("metric", ["Mean R2", "MSE", "Pearson"])
def test_ae_pairs_equal_scipy(metric):
    stats = pytest.importorskip("scipy.stats")
    results = _results(True)
    entries = CV.compare(results, metric)
    assert [e["direction"] for e in entries] == ["DNA -> RNA", "RNA -> DNA"]
    for e in entries:
        rows = [r for r in results if r["direction"] == e["direction"]]
        best = {m: max((r for r in rows if r["model"] == m), key=lambda r: r["mean_Mean R2"]) for m in ("ae", "vae", "knn")}
        assert e["best_ae"] == best["ae"]["param_value"]
        for key, other, name in (("ae_vs_vae", "vae", "VAE"), ("ae_vs_knn", "knn", "kNN")):
            a, b = best["ae"]["fold_metrics"][metric], best[other]["fold_metrics"][metric]
            want = stats.ttest_rel(a, b)
            c = e[key]
            assert (c["a"], c["b"], c["df"]) == ("AE", name, len(a) - 1)
            assert c["t"] == pytest.approx(float(want.statistic), rel=1e-12) and c["p"] == pytest.approx(float(want.pvalue), rel=1e-9, abs=1e-300)
            assert c["mean_a"] == pytest.approx(np.mean(a)) and c["mean_b"] == pytest.approx(np.mean(b))
            higher = metric != "MSE"
            better = "AE" if ((np.mean(a) > np.mean(b)) == higher) else name
            assert c["winner"] == (better if want.pvalue < 0.05 else None)
            assert set(c) == set(e["knn_vs_vae"])                                   # the pair format of the existing entries


def test_without_ae_rows_the_comparison_is_what_it_was():
    results = _results(False)
    for metric in ("Mean R2", "MSE"):
        entries = CV.compare(results, metric)
        with_ae = CV.compare(_results(True), metric)
        for e, f in zip(entries, with_ae):
            assert set(e) == {"direction", "metric", "best_knn", "best_vae", "knn_vs_vae", "vae_vs_mean", "best_knn_site", "knn_site_vs_vae"}
            assert {k: v for k, v in f.items() if k in e} == e                        # AE rows change nothing of the other entries
            assert set(f) - set(e) == {"best_ae", "ae_vs_vae", "ae_vs_knn"}
            rows = [r for r in results if r["direction"] == e["direction"]]
            knn = max((r for r in rows if r["model"] == "knn"), key=lambda r: r["mean_Mean R2"])
            vae = next(r for r in rows if r["model"] == "vae")
            assert e["knn_vs_vae"] == CV._pair("kNN", knn, "VAE", vae, metric) and e["best_knn"] == knn["param_value"]


def test_the_name_ae_is_not_a_model_to_ask_for():
    assert "ae" not in CV.MODELS and CV.AE_MODEL == "autoencoder" and CV.AE_ROW == "ae"
