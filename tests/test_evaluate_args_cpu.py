"""evaluate.check_args: every flag combination and range evaluate.py refuses is refused right after parsing, with its message, before
any data, checkpoint or device is touched; a full valid flag set passes."""
import pytest

import evaluate

REFUSED = [
    (["--knn-tune-out", "t.json"], "--knn-tune-out needs --knn-tune"),
    (["--knn-by-site"], "--knn-by-site needs --knn K or --knn-tune"),
    (["--clustering-out", "c.json"], "--clustering-out needs --clustering"),
    (["--clustering-pca", "2"], "--clustering-pca needs --clustering"),
    (["--clustering-tsne"], "--clustering-tsne needs --clustering"),
    (["--clustering", "--clustering-tsne", "--tsne-perplexity", "0"], "--tsne-perplexity must be positive and --tsne-iters at least 250"),
    (["--clustering", "--clustering-tsne", "--tsne-iters", "249"], "--tsne-perplexity must be positive and --tsne-iters at least 250"),
    (["--clustering", "--clustering-pca", "-1"], "--clustering-pca -1 outside [0, min(64, validation rows, features)]"),
    (["--downstream-out", "d.json"], "--downstream-out needs --downstream"),
    (["--downstream", "--downstream-folds", "1"], "--downstream-folds must be at least 2 and --downstream-epochs at least 1"),
    (["--downstream", "--downstream-epochs", "0"], "--downstream-folds must be at least 2 and --downstream-epochs at least 1"),
]
FULL = ["--knn", "5", "--knn-by-site", "--knn-tune", "--knn-tune-out", "t.json", "--clustering", "--clustering-pca", "2", "--clustering-tsne",
        "--tsne-iters", "250", "--clustering-out", "c.json", "--downstream", "--downstream-folds", "2", "--downstream-epochs", "3",
        "--downstream-out", "d.json", "--out", "o.json"]


@pytest.mark.parametrize("kind", ["multimodal", "rna2dna", "dna2rna"])
def test_refused_flag_sets_and_their_messages(kind):
    for argv, message in REFUSED:
        with pytest.raises(SystemExit) as e:
            evaluate.check_args(evaluate.build_parser(kind).parse_args(argv))
        assert str(e.value) == message, argv


@pytest.mark.parametrize("kind", ["multimodal", "rna2dna", "dna2rna"])
def test_valid_flag_sets_pass(kind):
    for argv in ([], FULL, ["--knn-tune", "--knn-by-site"], ["--clustering", "--clustering-pca", "64"]):
        assert evaluate.check_args(evaluate.build_parser(kind).parse_args(argv)) is None
