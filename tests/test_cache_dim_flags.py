"""--semantic-cache-dim: startup checks of the flag combinations."""

import argparse

import pytest

from aigw.cli.main import _check_cache_flags


def _args(**kw):
    base = dict(front="lean", gpu=True, semantic_cache=True, cache_scope="value",
                cache_ttl_s=0.0, cache_index_dtype="bf16", cache_candidates=1, workers=1)
    return argparse.Namespace(**{**base, **kw})


@pytest.mark.parametrize("kw, message", [
    (dict(cache_dim=576), "multiple of 128"),
    (dict(cache_dim=1152), "128..1024"),
    (dict(cache_dim=768, front="fast"), "fixed at 384"),
    (dict(cache_dim=768, cache_index_dtype="mxfp4"), "mxfp4"),
    (dict(cache_dim=768, cache_candidates=2), "candidates above 1"),
])
def test_rejected(kw, message):
    with pytest.raises(SystemExit, match=message):
        _check_cache_flags(_args(**kw))


@pytest.mark.parametrize("kw", [dict(cache_dim=768), dict(cache_dim=1024, cache_index_dtype="fp8"),
                                dict(cache_dim=512, cache_candidates=2)])
def test_accepted(kw):
    _check_cache_flags(_args(**kw))
