"""--semantic-cache-candidates: startup checks of the flag combinations."""

import argparse

import pytest

from aigw.cli.main import _check_cache_flags


def _args(**kw):
    base = dict(front="lean", gpu=True, semantic_cache=True, cache_scope="value",
                cache_ttl_s=0.0, cache_index_dtype="bf16", cache_candidates=1)
    return argparse.Namespace(**{**base, **kw})


@pytest.mark.parametrize("kw, message", [
    (dict(cache_candidates=2, front="fast"), "--front fast"),
    (dict(cache_candidates=8, cache_index_dtype="mxfp4"), "mxfp4"),
    (dict(cache_candidates=2, workers=2), "--workers 1"),
    (dict(cache_candidates=9), "1..8"),
])
def test_rejected(kw, message):
    with pytest.raises(SystemExit, match=message):
        _check_cache_flags(_args(**kw))


@pytest.mark.parametrize("kw", [dict(cache_candidates=2), dict(front="fast")])
def test_accepted(kw):
    _check_cache_flags(_args(**kw))
