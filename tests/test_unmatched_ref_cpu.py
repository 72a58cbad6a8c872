"""tests/unmatched_ref.py (float64 numpy) against what the reference's cluster_imputation_methods.py recorded in
tests/golden/unmatched_clustering.npz (tools/make_unmatched_fixture.py), and the conditions the fixture's seed was chosen by."""
import os

import numpy as np
import pytest

import unmatched_bounds as UB
import unmatched_ref as UR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unmatched_clustering.npz")
ROWS = [(st, m) for st in UR.SAMPLE_TYPES for m in UR.IMPUTERS]


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


def test_inputs_are_the_seeded_ones_and_the_seed_satisfies_its_conditions(fx):
    d = UR.inputs(int(fx["seed"]))
    for name, v in d.items():
        assert np.array_equal(v, fx[name]), name
    assert UR.conditions(d) == (True, True, True)
    assert d["train_rna"].shape == (96, UR.A) and d["rna_only"].shape == (40, UR.A) and d["dna_only"].shape == (40, UR.D)
    assert (d["rna_only_site"] < 0).sum() == 1 and (d["dna_only_site"] < 0).sum() == 1          # one sample of an unknown site each
    assert np.bincount(d["train_site"]).min() == 3 < UR.K                                      # one site with fewer than k training rows


@pytest.mark.parametrize("st,method", ROWS)
def test_restatement_equals_the_reference(fx, st, method):
    d = UR.inputs(int(fx["seed"]))
    key = f"{st}/{method}/"
    F_rec, labels = fx[key + "features"], fx[key + "labels"]
    x, site = UR.known(d, st)
    assert np.array_equal(labels, site) and F_rec.dtype == np.float32 and F_rec.shape == (39, UR.A + UR.D)
    F = UR.features(d, st, method, "reference")
    n0 = x.shape[1]
    assert np.array_equal(F[:, :n0], F_rec[:, :n0])                                            # the original block: the same bits
    T = UB.block_tol(F_rec[:, n0:], method, UR.K, log1p_on_top=st == "DNA-only", train_rows=len(d["train_site"]))
    assert np.all(np.abs(F[:, n0:].astype(np.float64) - F_rec[:, n0:]) <= T)
    if method == "mean":
        assert np.all(np.ptp(F_rec[:, n0:], axis=0) == 0)
    Tfull = np.concatenate([np.zeros((len(F), n0)), T], axis=1)
    z64, tol = UB.z_tol_record(F_rec, Tfull, 1)
    assert np.all(np.abs(fx[key + "Z"].astype(np.float64) - z64) <= tol)                       # sklearn's own Z around the float64 z
    j = UR.judged(F_rec, labels)
    assert j["nh"] == float(fx[key + "nh"]) and j["pca_nh"] == float(fx[key + "pca_nh"])       # the seed decides every neighbour
    # sklearn's silhouette on its float32 Z: rows within |Z_rec - z64| of the restatement's
    for Zr, name in ((fx[key + "Z"], "sil"),):
        err = np.sqrt(((Zr.astype(np.float64) - z64) ** 2).sum(axis=1))
        lo, hi = UB.silhouette_interval(z64, labels, err, 1)
        assert lo <= float(fx[key + name]) <= hi and lo <= j[name] <= hi
    assert abs(j["explained"] - float(fx[key + "explained"])) <= 1e-5 * j["explained"]          # float32 SVD of sklearn against float64
    assert abs(j["pca_sil"] - float(fx[key + "pca_sil"])) <= 1e-4


def test_consistent_scaling_differs_only_where_it_should():
    d = UR.inputs(0)
    for method in UR.IMPUTERS:
        r, c = UR.features(d, "RNA-only", method, "reference"), UR.features(d, "RNA-only", method, "consistent")
        assert np.array_equal(c[:, :UR.A], np.log1p(r[:, :UR.A]))
        r, c = UR.features(d, "DNA-only", method, "reference"), UR.features(d, "DNA-only", method, "consistent")
        assert np.array_equal(r[:, :UR.D], c[:, :UR.D]) and np.array_equal(r[:, UR.D:], np.log1p(c[:, UR.D:]))
