"""The command-line surface of the five tools, option by option: every action's option strings, default, choices, nargs and type, in parser
order, against a table taken from the parsers as they stood before their shared arguments moved into hostlib (INPUT_DIM_A, INPUT_DIM_B
and LATENT_DIM unset) -- and the three environment overrides still reach all five."""
import pytest

import cluster_unmatched
import cross_validate
import evaluate
import reconstruct
import trainer

KINDS = ("multimodal", "dna2rna", "rna2dna")
ENV = {"INPUT_DIM_A": ("--input-dim-a", 782), "INPUT_DIM_B": ("--input-dim-b", 572), "LATENT_DIM": ("--latent-dim", 20)}

PARSERS = {'trainer': [(('-h', '--help'), '==SUPPRESS==', None, 0, None),
             (('--data',), None, None, None, None),
             (('--samples',), 262144, None, None, 'int'),
             (('--input-dim-a',), 782, None, None, 'int'),
             (('--input-dim-b',), 572, None, None, 'int'),
             (('--n-sites',), 24, None, None, 'int'),
             (('--latent-dim',), 20, None, None, 'int'),
             (('--batch-size',), 4096, None, None, 'int'),
             (('--epochs',), 200, None, None, 'int'),
             (('--precision',), 'bf16', ('bf16', 'fp32'), None, None),
             (('--input-dtype',), 'fp32', ('fp32', 'bf16'), None, None),
             (('--checkpoint-dir',), 'checkpoints', None, None, None),
             (('--resume',), None, None, None, None),
             (('--save-state',), None, None, None, None),
             (('--eager',), False, None, 0, None),
             (('--backend',), 'nccl', None, None, None),
             (('--single-device',), False, None, 0, None),
             (('--log-json',), None, None, None, None)],
 'evaluate': [(('-h', '--help'), '==SUPPRESS==', None, 0, None),
              (('--data',), None, None, None, None),
              (('--samples',), 262144, None, None, 'int'),
              (('--input-dim-a',), 782, None, None, 'int'),
              (('--input-dim-b',), 572, None, None, 'int'),
              (('--n-sites',), 24, None, None, 'int'),
              (('--latent-dim',), 20, None, None, 'int'),
              (('--batch-size',), 4096, None, None, 'int'),
              (('--precision',), 'bf16', ('bf16', 'fp32'), None, None),
              (('--input-dtype',), 'fp32', ('fp32', 'bf16'), None, None),
              (('--checkpoint',), None, None, None, None),
              (('--checkpoint-dir',), 'checkpoints', None, None, None),
              (('--seed',), 42, None, None, 'int'),
              (('--knn',), 0, None, None, 'int'),
              (('--knn-by-site',), False, None, 0, None),
              (('--knn-tune',), False, None, 0, None),
              (('--knn-tune-out',), None, None, None, None),
              (('--out',), None, None, None, None),
              (('--clustering',), False, None, 0, None),
              (('--clustering-out',), None, None, None, None),
              (('--clustering-pca',), 0, None, None, 'int'),
              (('--clustering-tsne',), False, None, 0, None),
              (('--tsne-perplexity',), 30.0, None, None, 'float'),
              (('--tsne-iters',), 1000, None, None, 'int'),
              (('--downstream',), False, None, 0, None),
              (('--downstream-folds',), 5, None, None, 'int'),
              (('--downstream-epochs',), 100, None, None, 'int'),
              (('--downstream-out',), None, None, None, None)],
 'cross_validate': [(('-h', '--help'), '==SUPPRESS==', None, 0, None),
                    (('--folds',), 10, None, None, 'int'),
                    (('--subset',), 0.1, None, None, 'float'),
                    (('--neighbors',), [5, 10], None, '+', 'int'),
                    (('--epochs',), 200, None, None, 'int'),
                    (('--batch-size',), 32, None, None, 'int'),
                    (('--data',), None, None, None, None),
                    (('--samples',), 262144, None, None, 'int'),
                    (('--input-dim-a',), 782, None, None, 'int'),
                    (('--input-dim-b',), 572, None, None, 'int'),
                    (('--n-sites',), 24, None, None, 'int'),
                    (('--latent-dim',), 20, None, None, 'int'),
                    (('--precision',), 'bf16', ('bf16', 'fp32'), None, None),
                    (('--input-dtype',), 'fp32', ('fp32', 'bf16'), None, None),
                    (('--seed',), 42, None, None, 'int'),
                    (('--models',), ['mean', 'knn', 'vae'], None, '+', None),
                    (('--knn-by-site',), False, None, 0, None),
                    (('--autoencoder',), False, None, 0, None),
                    (('--eager',), False, None, 0, None),
                    (('--out',), None, None, None, None)],
 'reconstruct': [(('-h', '--help'), '==SUPPRESS==', None, 0, None),
                 (('--data-dir',), 'data', None, None, None),
                 (('--timestamp',), None, None, None, None),
                 (('--checkpoint-dir',), 'checkpoints', None, None, None),
                 (('--checkpoint-rna2dna',), None, None, None, None),
                 (('--checkpoint-dna2rna',), None, None, None, None),
                 (('--input-dim-a',), 782, None, None, 'int'),
                 (('--input-dim-b',), 572, None, None, 'int'),
                 (('--latent-dim',), 20, None, None, 'int'),
                 (('--draws',), 1, None, None, 'int'),
                 (('--dna-sites',), 'none', ('none', 'all'), None, None),
                 (('--batch-size',), 4096, None, None, 'int'),
                 (('--precision',), 'bf16', ('bf16', 'fp32'), None, None),
                 (('--seed',), 42, None, None, 'int'),
                 (('--synthetic',), 0, None, None, 'int')],
 'cluster_unmatched': [(('-h', '--help'), '==SUPPRESS==', None, 0, None),
                       (('--methods',), None, ('mean', 'knn', 'cond_knn', 'vae'), '+', None),
                       (('--neighbors',), 5, None, None, 'int'),
                       (('--scaling',), 'consistent', ('consistent', 'reference'), None, None),
                       (('--data-dir',), 'data', None, None, None),
                       (('--from-reconstruction',), None, None, None, None),
                       (('--no-tsne',), False, None, 0, None),
                       (('--tsne-iters',), 1000, None, None, 'int'),
                       (('--seed',), 42, None, None, 'int'),
                       (('--out',), None, None, None, None),
                       (('--embeddings-out',), None, None, None, None),
                       (('--synthetic',), 0, None, None, 'int'),
                       (('--checkpoint-dir',), 'checkpoints', None, None, None),
                       (('--checkpoint-rna2dna',), None, None, None, None),
                       (('--checkpoint-dna2rna',), None, None, None, None),
                       (('--input-dim-a',), 782, None, None, 'int'),
                       (('--input-dim-b',), 572, None, None, 'int'),
                       (('--latent-dim',), 20, None, None, 'int'),
                       (('--batch-size',), 4096, None, None, 'int'),
                       (('--precision',), 'bf16', ('bf16', 'fp32'), None, None)]}

BUILDERS = [("trainer", trainer.build_parser, k) for k in KINDS] + [("evaluate", evaluate.build_parser, k) for k in KINDS] \
    + [("cross_validate", cross_validate.build_parser, None), ("reconstruct", reconstruct.build_parser, None),
       ("cluster_unmatched", cluster_unmatched.build_parser, None)]


def describe(ap):
    return [(tuple(a.option_strings), a.default, None if a.choices is None else tuple(a.choices), a.nargs, getattr(a.type, "__name__", None))
            for a in ap._actions]


@pytest.mark.parametrize("name,build,kind", BUILDERS, ids=[f"{n}-{k}" if k else n for n, _, k in BUILDERS])
def test_every_option_is_as_it_was(name, build, kind, monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    assert describe(build(kind) if kind else build()) == PARSERS[name]


@pytest.mark.parametrize("name,build,kind", BUILDERS, ids=[f"{n}-{k}" if k else n for n, _, k in BUILDERS])
def test_the_environment_overrides_reach_every_parser(name, build, kind, monkeypatch):
    values = {"INPUT_DIM_A": 11, "INPUT_DIM_B": 7, "LATENT_DIM": 3}
    for var, v in values.items():
        monkeypatch.setenv(var, str(v))
    want = {ENV[var][0]: v for var, v in values.items()}
    expected = [(opts, want.get(opts[0], default), choices, nargs, typ) for opts, default, choices, nargs, typ in PARSERS[name]]
    assert sum(opts[0] in want for opts, *_ in PARSERS[name]) == 3
    assert describe(build(kind) if kind else build()) == expected
