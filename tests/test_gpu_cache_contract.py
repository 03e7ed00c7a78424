"""The host contract the eight semantic-cache lookup entry points share:
argument checks, the `now` range, tag alignment, views, empty calls. One
table drives every entry point, with and without tags where it takes them
optionally, through the same cases.

Shapes are the smallest that reach each check: 16 planted rows behind 4
offset rows (copies of query 0's winner), dim 128 for the narrow entry points
and 640 for the wide ones, 3 queries, k = 2. What the kernels compute is
checked elsewhere (test_gpu_cache_*.py); here a result only has to be the
planted winners."""

import functools
import itertools

import pytest
import torch

import kernel_checks as kc
from aigw.ops import mxfp4_ref as mx
from kernel_checks import NEVER

pytestmark = pytest.mark.gpu

NOW = 1000
WINNERS = [3, 9, 14]  # rows of the 16-row view; +4 in the whole allocation
K = 2


@pytest.fixture(scope="module")
def hip():
    import aigw_hip

    return aigw_hip


class Op:
    """One entry point: its row width, a width just outside its range, the
    index format, and whether the three tag tensors are absent, optional or
    required."""

    def __init__(self, name, dim, bad_dim, other_dim, tags, mxfp4=False, k=None):
        self.name, self.dim, self.bad_dim, self.other_dim = name, dim, bad_dim, other_dim
        self.tags, self.mxfp4, self.k = tags, mxfp4, k

    def parts(self, rows):
        """bf16 rows [n, dim] (CPU) -> the index tensors of a call, on the GPU."""
        if not self.mxfp4:
            return (rows.cuda(),)
        return tuple(torch.from_numpy(a).cuda()
                     for a in mx.quantize(rows.to(torch.float64).numpy()))

    def queries(self, rows):
        return rows.to(torch.float8_e4m3fn if self.mxfp4 else torch.bfloat16).cuda()

    def __call__(self, hip, parts, q, tags=()):
        args = (*parts, q) if self.k is None else (*parts, q, self.k)
        return getattr(hip, self.name)(*args, *tags)

    def shape(self, n_q):
        return (n_q,) if self.k is None else (n_q, self.k)


OPS = [
    Op("cache_topk", 128, 640, 256, "none"),
    Op("cache_topk_scoped", 128, 640, 256, "required"),
    Op("cache_topk_k", 128, 640, 256, "optional", k=K),
    Op("cache_topk_wide", 640, 512, 768, "optional"),
    Op("cache_topk_wide_tiled", 640, 512, 768, "optional"),
    Op("cache_topk_mxfp4", 128, 640, 256, "none", mxfp4=True),
    Op("cache_topk_mxfp4_scoped", 128, 640, 256, "required", mxfp4=True),
    Op("cache_topk_mxfp4_wide", 640, 512, 768, "optional", mxfp4=True),
]
# every way to call an entry point: (op, tagged)
CALLS = [(op, tagged) for op in OPS for tagged in (False, True)
         if (tagged and op.tags != "none") or (not tagged and op.tags != "required")]
TAGGED = [op for op in OPS if op.tags != "none"]
OPTIONAL = [op for op in OPS if op.tags == "optional"]


def _ids(items):
    return [f"{i[0].name}{'-tagged' if i[1] else ''}" if isinstance(i, tuple) else i.name
            for i in items]


class Case:
    """20 rows of one entry point's width: 4 offset rows in front of 16
    planted ones, the three queries, and tags under which every row is
    eligible for its query (two row scopes; queries 0 and 2 ask for their
    winner's scope, query 1 for any)."""

    def __init__(self, op, dim):
        index, q_rows = kc.planted_case(16, dim, torch.bfloat16, WINNERS, seed=90 + dim)
        rows = torch.cat([q_rows[:1].expand(4, -1), index])
        self.parts = op.parts(rows)
        self.q = op.queries(q_rows)
        s0, s1 = kc.scope_ids(2, seed=91)
        scope_of = [s0 if r % 2 else s1 for r in range(16)]
        self.row_scope = torch.tensor([scope_of[WINNERS[0]]] * 4 + scope_of).cuda()
        self.row_expiry = torch.full((20,), NEVER, dtype=torch.int32).cuda()
        self.q_scope = torch.tensor([scope_of[WINNERS[0]], 0, scope_of[WINNERS[2]]]).cuda()
        assert self.row_scope.data_ptr() % 32 == 0 and self.row_expiry.data_ptr() % 16 == 0

    def tags(self, tagged, rows=slice(None), n_q=None, now=NOW):
        if not tagged:
            return ()
        qs = self.q_scope if n_q is None else self.q_scope[:1].expand(n_q).contiguous()
        return (self.row_scope[rows], self.row_expiry[rows], qs, now)

    def rows(self, sl):
        return tuple(p[sl] for p in self.parts)


@functools.lru_cache(maxsize=None)
def _case(op, dim=None):
    return Case(op, dim or op.dim)


def _winners(op, idx, offset=0):
    got = idx.cpu().tolist()
    return [r[0] for r in got] if op.k else got, [w + offset for w in WINNERS]


@pytest.mark.parametrize("op,tagged", CALLS, ids=_ids(CALLS))
def test_wrong_rank_and_dim_mismatch(hip, op, tagged):
    c = _case(op)
    tags = c.tags(tagged)
    got, want = _winners(op, op(hip, c.parts, c.q, tags)[1], 4)
    assert got[1:] == want[1:] and (got[0] < 4 or got[0] == want[0])
    first = c.parts[0]
    for bad in (first.reshape(-1), first[None]):
        with pytest.raises(RuntimeError):
            op(hip, (bad, *c.parts[1:]), c.q, tags)
    for bad in (c.q.reshape(-1), c.q[None]):
        with pytest.raises(RuntimeError):
            op(hip, c.parts, bad, tags)
    other = _case(op, op.other_dim)  # another width the entry point serves
    op(hip, other.parts, other.q, tags)
    with pytest.raises(RuntimeError):
        op(hip, c.parts, other.q, tags)
    with pytest.raises(RuntimeError):
        op(hip, other.parts, c.q, tags)


@pytest.mark.parametrize("op,tagged", CALLS, ids=_ids(CALLS))
def test_dim_out_of_range(hip, op, tagged):
    c = _case(op, op.bad_dim)
    with pytest.raises(RuntimeError):
        op(hip, c.parts, c.q, c.tags(tagged))


@pytest.mark.parametrize("op,tagged", CALLS, ids=_ids(CALLS))
def test_query_count_limit(hip, op, tagged):
    c = _case(op)
    q257 = c.q[:1].expand(257, -1).contiguous()
    with pytest.raises(RuntimeError):
        op(hip, c.parts, q257, c.tags(tagged, n_q=257))
    hi, idx = op(hip, c.parts, q257[:256], c.tags(tagged, n_q=256))
    assert hi.shape == op.shape(256) and idx.shape == op.shape(256)


@pytest.mark.parametrize("op,tagged", CALLS, ids=_ids(CALLS))
def test_empty_calls(hip, op, tagged):
    c = _case(op)
    hi, idx = op(hip, c.parts, c.q[:0], c.tags(tagged, n_q=0))
    assert hi.shape == op.shape(0) and idx.shape == op.shape(0)
    assert hi.dtype == torch.int64 and idx.dtype == torch.int32
    hi, idx = op(hip, c.rows(slice(0, 0)), c.q, c.tags(tagged, rows=slice(0, 0)))
    assert hi.shape == op.shape(3) and idx.shape == op.shape(3)
    assert hi.dtype == torch.int64 and idx.dtype == torch.int32
    assert (hi == 0).all() and (idx == -1).all()


@pytest.mark.parametrize("op", TAGGED, ids=_ids(TAGGED))
def test_now_must_fit_int32(hip, op):
    c = _case(op)
    for ok in (2 ** 31 - 1, -2 ** 31):
        op(hip, c.parts, c.q, c.tags(True, now=ok))
    for bad in (2 ** 31, -2 ** 31 - 1):
        with pytest.raises(RuntimeError):
            op(hip, c.parts, c.q, c.tags(True, now=bad))


@pytest.mark.parametrize("op", TAGGED, ids=_ids(TAGGED))
def test_misaligned_tag_views_are_refused(hip, op):
    c = _case(op)
    rs, re, qs, now = c.tags(True)
    parts = tuple(p[1:].clone() for p in c.parts)
    rs_ok, re_ok = rs[1:].clone(), re[1:].clone()
    assert rs_ok.data_ptr() % 32 == 0 and re_ok.data_ptr() % 16 == 0
    assert rs[1:].data_ptr() % 32 and re[1:].data_ptr() % 16
    op(hip, parts, c.q, (rs_ok, re_ok, qs, now))
    for bad_rs, bad_re in [(rs[1:], re[1:]), (rs[1:], re_ok), (rs_ok, re[1:])]:
        with pytest.raises(RuntimeError):
            op(hip, parts, c.q, (bad_rs, bad_re, qs, now))


@pytest.mark.parametrize("op", TAGGED, ids=_ids(TAGGED))
def test_views_from_row_4_are_served(hip, op):
    c = _case(op)
    view = slice(4, None)
    hi, idx = op(hip, c.rows(view), c.q, c.tags(True, rows=view))
    got, want = _winners(op, idx)
    assert got == want  # numbered relative to the view
    # the same rows as allocations of their own give the same keys
    rs, re, qs, now = c.tags(True, rows=view)
    hi2, idx2 = op(hip, tuple(p.clone() for p in c.rows(view)), c.q,
                   (rs.clone(), re.clone(), qs, now))
    assert torch.equal(hi, hi2) and torch.equal(idx, idx2)


@pytest.mark.parametrize("op", OPTIONAL, ids=_ids(OPTIONAL))
def test_tags_come_together_or_not_at_all(hip, op):
    c = _case(op)
    names = ("row_scope", "row_expiry", "q_scope")
    given = dict(zip(names, c.tags(True)[:3]))
    args = (*c.parts, c.q) if op.k is None else (*c.parts, c.q, op.k)
    fn = getattr(hip, op.name)
    fn(*args, **given, now=NOW)
    for n in (1, 2):
        for some in itertools.combinations(names, n):
            with pytest.raises(RuntimeError):
                fn(*args, **{k: given[k] for k in some}, now=NOW)
