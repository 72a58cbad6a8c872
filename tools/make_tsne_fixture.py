"""Writes tests/golden/tsne.npz from scikit-learn (1.7.2 when the committed file was made): what tests/test_tsne_ref_cpu.py holds
tests/tsne_ref.py to, and the spread of sklearn's own t-SNE runs that tests/test_tsne_fit_gpu.py holds the device fit to.

    python tools/make_tsne_fixture.py

Small cases (name_*): rows X, sklearn's neighbour graph (idx, d2 as the fp32 it searches on), _binary_search_perplexity's conditional P,
_joint_probabilities_nn's CSR P, and _kl_divergence_bh(angle=0) -- error and gradient, fp32 inside sklearn -- at embeddings of scale 1e-4,
1 and 10.  Blobs record (blobs_*): TSNE(2, perplexity=30, method="barnes_hut", angle=0.0) on tsne_ref.blobs() with init="pca" once and
init="random" under seven seeds; per run the KL recomputed by tsne_ref from the embedding, trustworthiness(X, Y, n_neighbors=5) and the
silhouette by class (and the first run's embedding, blobs_Y_pca).  grad_rel_seen / kl_rel_seen: the largest |sklearn - tsne_ref| /
max|grad| and |kl - kl_ref| / kl_ref over the small cases; sklearn's gradient is fp32 inside, summed in its tree's order, so the
test's tolerances grad_rel_tol / kl_rel_tol are these two rounded up to the next power of ten (1e-5 both when the file was made)."""
import os
import sys

import numpy as np
import sklearn
from scipy.sparse import csr_matrix
from sklearn.manifold import TSNE, _t_sne, _utils, trustworthiness
from sklearn.neighbors import NearestNeighbors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tsne_ref as TR  # noqa: E402

CASES = {"a": dict(n=80, f=5, perplexity=5.0, seed=1), "b": dict(n=150, f=8, perplexity=12.0, seed=2), "c": dict(n=40, f=3, perplexity=30.0, seed=3)}
SCALES = (1e-4, 1.0, 10.0)


def small_case(n, f, perplexity, seed):
    g = np.random.default_rng(seed)
    X = (g.standard_normal((n, f)) + 3.0 * g.standard_normal((4, f))[np.arange(n) % 4]).astype(np.float32)
    k = min(n - 1, int(3.0 * perplexity + 1))
    graph = NearestNeighbors(n_neighbors=k).fit(X).kneighbors_graph(mode="distance")
    graph.data **= 2
    graph.sort_indices()
    d2 = graph.data.reshape(n, -1).astype(np.float32)
    cond = _utils._binary_search_perplexity(d2, perplexity, 0)
    P = _t_sne._joint_probabilities_nn(graph, perplexity, 0)
    P.sort_indices()
    out = dict(X=X, perplexity=np.float64(perplexity), idx=graph.indices.reshape(n, -1).astype(np.int32), d2=d2, cond=np.asarray(cond, np.float64),
               indptr=P.indptr.astype(np.int64), indices=P.indices.astype(np.int64), data=P.data.astype(np.float64))
    seen = [0.0, 0.0]
    for s, scale in enumerate(SCALES):
        Y = (scale * g.standard_normal((n, 2))).astype(np.float32)
        kl, grad = _t_sne._kl_divergence_bh(Y.ravel(), csr_matrix((P.data, P.indices, P.indptr), shape=(n, n)), 1, n, 2, angle=0.0, num_threads=1)
        ref = TR.gradient(Y, out["indptr"], out["indices"], out["data"].astype(np.float32))
        seen[0] = max(seen[0], float(np.abs(grad.reshape(n, 2) - ref["grad"]).max() / np.abs(ref["grad"]).max()))
        seen[1] = max(seen[1], abs(kl - ref["kl"]) / abs(ref["kl"]))
        out.update({f"Y{s}": Y, f"kl{s}": np.float64(kl), f"grad{s}": grad.reshape(n, 2).astype(np.float64)})
    return out, seen


def blobs_record():
    X, labels = TR.blobs()
    P = TR.joint_probabilities(X, 30.0)
    rows, first = [], None
    for init, seed in [("pca", 0)] + [("random", s) for s in range(1, 8)]:
        t = TSNE(2, perplexity=30.0, method="barnes_hut", angle=0.0, init=init, random_state=seed)
        Y = t.fit_transform(X)
        first = Y if first is None else first
        rows.append((TR.kl_of(P, Y), trustworthiness(X, Y, n_neighbors=5), TR.silhouette(Y, labels), t.kl_divergence_, t.n_iter_))
        print(init, seed, rows[-1], flush=True)
    r = np.array(rows, np.float64)
    return dict(blobs_Y_pca=np.asarray(first, np.float32), blobs_kl=r[:, 0], blobs_trust=r[:, 1], blobs_silhouette=r[:, 2], blobs_sklearn_kl=r[:, 3], blobs_n_iter=r[:, 4])


def main():
    out, seen = {}, [0.0, 0.0]
    for name, kw in CASES.items():
        c, s = small_case(**kw)
        out.update({f"{name}_{k}": v for k, v in c.items()})
        seen = [max(a, b) for a, b in zip(seen, s)]
    for name, v in zip(("grad", "kl"), seen):
        out[f"{name}_rel_seen"] = np.float64(v)
        out[f"{name}_rel_tol"] = np.float64(10.0 ** np.ceil(np.log10(v)))
    out["sklearn_version"] = np.array(sklearn.__version__)
    out.update(blobs_record())
    path = os.path.join(ROOT, "tests", "golden", "tsne.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; grad_rel_seen", seen)


if __name__ == "__main__":
    main()
