"""The 16-bit index search on the MI355X (grit_knn16_topk through index_ops.knn16_topk and rag.DistributedIndex), every case for a bf16
and an fp16 index.  The reference is numpy fp64 on the 16-bit values of the index and the fp32 values of the queries; where the data
make every partial sum exact in fp32 the comparison is bit for bit, indices included (numpy's stable sort by (-score, column))."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
FORMATS = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="fp16")]


def _index(e: np.ndarray, dt, ld=None):
    """[H, N] values -> the index tensor on the GPU (contiguous, or a view of a [H, ld] buffer) and its 16-bit values in fp64"""
    t = torch.from_numpy(np.ascontiguousarray(e, np.float32)).to(DEV).to(dt)
    if ld is not None:
        buf = torch.full((e.shape[0], ld), float("nan"), dtype=dt, device=DEV)      # what lies between the rows must not matter
        buf[:, :e.shape[1]] = t
        t = buf[:, :e.shape[1]]
    return t, t.double().cpu().numpy()


def _search(q: np.ndarray, et: torch.Tensor, k: int):
    from gritlm_amd import index_ops
    sc, ix = index_ops.knn16_topk(torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(DEV), et, k)
    torch.cuda.synchronize()
    return sc.cpu().numpy(), ix.cpu().numpy()


def _exact_reference(q, e64, k):
    """scores that are exact in fp32: the k best by numpy's stable sort of (-score, column)"""
    ref = q.astype(np.float64) @ e64
    assert np.array_equal(ref, ref.astype(np.float32).astype(np.float64))
    order = np.argsort(-ref, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(ref, order, axis=1).astype(np.float32), order


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _unit(rng, rows, cols):
    x = rng.standard_normal((rows, cols))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _condition4(sc, ix, q, e64, k, label=""):
    """every returned score within tol of the reference score of its index; non-increasing; indices distinct and in range; no column
    left out exceeds the k-th returned score by more than 2 tol.  tol = 1.02 * 3H * 2^-24 * sum_h |q_h e_h|: the first-order bound for
    any fp32 summation order of the 3H exact products."""
    Q, H = q.shape
    N = e64.shape[1]
    ref = q.astype(np.float64) @ e64
    tol = 1.02 * 3 * H * 2.0 ** -24 * (np.abs(q).astype(np.float64) @ np.abs(e64))
    assert sc.shape == (Q, k) and ix.shape == (Q, k)
    assert ((ix >= 0) & (ix < N)).all()
    err = np.abs(sc.astype(np.float64) - np.take_along_axis(ref, ix, axis=1)) / np.take_along_axis(tol, ix, axis=1)
    print(f"knn16 {label}: largest error / tol = {float(err.max()):.4f}")
    assert (err <= 1.0).all(), float(err.max())
    assert (np.diff(sc, axis=1) <= 0).all()
    for r in range(Q):
        assert len(set(ix[r].tolist())) == k
        left = np.ones(N, bool)
        left[ix[r]] = False
        assert (ref[r, left] <= float(sc[r, k - 1]) + 2 * tol[r, left]).all()


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("dt", FORMATS)
def test_query_pieces_are_exact(dt):
    """every index column is a single +-1, so score(n) = +-q[h(n)]: a dropped or mis-scaled piece of the three-way split cannot pass"""
    rng = np.random.default_rng(11)
    Q, H, N = 4, 64, 300
    q = (rng.integers(2 ** 23, 2 ** 24, (Q, H)) * 2.0 ** -24 * rng.choice([-1.0, 1.0], (Q, H))).astype(np.float32)      # 24-bit mantissas in [0.5, 1)
    if dt == torch.bfloat16:
        q[3] = (q[3].astype(np.float64) * 2.0 ** rng.integers(-20, 21, H)).astype(np.float32)                            # a row mixing 2^-20 .. 2^20
    e = np.zeros((H, N), np.float32)
    e[rng.integers(0, H, N), np.arange(N)] = rng.choice([-1.0, 1.0], N)
    et, e64 = _index(e, dt)
    ref_sc, ref_ix = _exact_reference(q, e64, N)
    sc, ix = _search(q, et, N)
    assert np.array_equal(_bits(sc), _bits(ref_sc))
    assert np.array_equal(ix, ref_ix)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.fixture(scope="module")
def small_integers():
    rng = np.random.default_rng(12)
    return rng.integers(-8, 9, (33, 40)).astype(np.float32), rng.integers(-8, 9, (40, 4099)).astype(np.float32)


@pytest.mark.parametrize("k", [1, 5, 100])
@pytest.mark.parametrize("dt", FORMATS)
def test_exact_sums_ties_tails_and_both_staging_paths(small_integers, dt, k):
    """integers in [-8, 8]: every partial sum is exact, ties abound; H = 40 and N = 4099 leave a K tail and an N tail; the contiguous
    tensor has an odd row stride (general staging), the view a row stride of 4160 (aligned staging)"""
    q, e = small_integers
    general, e64 = _index(e, dt)
    aligned, _ = _index(e, dt, ld=4160)
    assert general.stride(0) == 4099 and aligned.stride(0) == 4160 and aligned.data_ptr() % 16 == 0
    ref_sc, ref_ix = _exact_reference(q, e64, k)
    sc_g, ix_g = _search(q, general, k)
    sc_a, ix_a = _search(q, aligned, k)
    assert np.array_equal(_bits(sc_g), _bits(ref_sc)) and np.array_equal(ix_g, ref_ix)
    assert np.array_equal(_bits(sc_a), _bits(ref_sc)) and np.array_equal(ix_a, ref_ix)
    assert np.array_equal(_bits(sc_g), _bits(sc_a)) and np.array_equal(ix_g, ix_a)


@pytest.mark.parametrize("dt", FORMATS)
def test_general_staging_at_every_row_offset(small_integers, dt):
    """the index as a view that starts 1 .. 8 elements into a buffer with an even row stride: every 2-byte offset of a row start from
    a 16-byte boundary, each against the same exact reference"""
    q, e = small_integers
    e = e[:, :600]
    ref_sc = ref_ix = None
    for off in range(1, 9):
        buf = torch.full((e.shape[0], 616), float("nan"), dtype=dt, device=DEV)
        buf[:, off:off + 600] = torch.from_numpy(e).to(DEV).to(dt)
        et = buf[:, off:off + 600]
        if ref_sc is None:
            ref_sc, ref_ix = _exact_reference(q, et.double().cpu().numpy(), 7)
        sc, ix = _search(q, et, 7)
        assert np.array_equal(_bits(sc), _bits(ref_sc)) and np.array_equal(ix, ref_ix), off


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("dt", FORMATS)
def test_strip_and_chunk_seams_with_distinct_scores(dt):
    """query j is (66049, 257, 1) on rows 3j .. 3j+2, which hold the base-257 digits (minus 128) of N distinct codes: all N scores of a
    query are distinct and exact.  The two largest sit on columns 0 and N - 1, the rest are spread by a seeded permutation."""
    rng = np.random.default_rng(13)
    Q, H, N, k = 3, 64, 300001, 100
    e = rng.integers(-128, 129, (H, N)).astype(np.float32)
    q = np.zeros((Q, H), np.float32)
    for j in range(Q):
        q[j, 3 * j:3 * j + 3] = (66049.0, 257.0, 1.0)
        codes = np.sort(rng.choice(257 ** 3, N, replace=False))[::-1]
        cols = np.concatenate(([0, N - 1], 1 + rng.permutation(N - 2)))
        placed = np.empty(N, np.int64)
        placed[cols] = codes
        e[3 * j] = placed // 66049 - 128
        e[3 * j + 1] = placed // 257 % 257 - 128
        e[3 * j + 2] = placed % 257 - 128
    et, e64 = _index(e, dt)
    ref_sc, ref_ix = _exact_reference(q, e64, k)
    assert (ref_ix[:, 0] == 0).all() and (ref_ix[:, 1] == N - 1).all() and (np.diff(ref_sc, axis=1) < 0).all()
    sc, ix = _search(q, et, k)
    assert np.array_equal(ix, ref_ix)
    assert np.array_equal(_bits(sc), _bits(ref_sc))


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("Q,N,H,k", [(5, 10000, 256, 10), (32, 70000, 128, 10), (2, 37, 64, 37), (1, 3001, 4096, 10)])
@pytest.mark.parametrize("dt", FORMATS)
def test_realistic_unit_norm_data(dt, Q, N, H, k):
    rng = np.random.default_rng(14)
    q = _unit(rng, Q, H)
    et, e64 = _index(_unit(rng, N, H).T, dt)
    sc, ix = _search(q, et, k)
    _condition4(sc, ix, q, e64, k, f"[{Q},{N},{H},{k}]")


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("dt", FORMATS)
def test_rows_are_independent_and_calls_are_reproducible(dt):
    rng = np.random.default_rng(15)
    Q, N, H, k = 33, 5000, 128, 10
    q = _unit(rng, Q, H)
    et, _ = _index(_unit(rng, N, H).T, dt)
    sc, ix = _search(q, et, k)
    sc2, ix2 = _search(q, et, k)
    assert np.array_equal(_bits(sc), _bits(sc2)) and np.array_equal(ix, ix2)                      # two calls
    sc1, ix1 = _search(q[20:21], et, k)
    assert np.array_equal(_bits(sc1[0]), _bits(sc[20])) and np.array_equal(ix1[0], ix[20])       # alone == as row 20 of 33
    qn = q.copy()
    qn[7] = np.nan
    scn, ixn = _search(qn, et, k)                                                                  # ... and the call returns
    keep = np.arange(Q) != 7
    assert np.array_equal(_bits(scn[keep]), _bits(sc[keep])) and np.array_equal(ixn[keep], ix[keep])


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("Q,N,H,k", [(3, 5000, 64, 1024), (2, 1, 64, 1)])
@pytest.mark.parametrize("dt", FORMATS)
def test_limits_of_k(dt, Q, N, H, k):
    rng = np.random.default_rng(16)
    q = _unit(rng, Q, H)
    et, e64 = _index(_unit(rng, N, H).T, dt)
    sc, ix = _search(q, et, k)
    _condition4(sc, ix, q, e64, k, f"[{Q},{N},{H},{k}]")


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("dt", FORMATS)
def test_distributed_index_searches_a_half_index_in_place(dt, tmp_path):
    from gritlm_amd import rag
    exp = json.load(open(os.path.join(HERE, "golden", "rag_index", "expected.json")))
    passages = [p for p in exp["loaded"] if p is not None]
    dim, N = exp["dim"], len(passages)
    idx = rag.DistributedIndex(dtype=dt)
    idx.init_embeddings(passages, dim)
    emb = idx.embeddings
    assert emb.is_cuda and emb.dtype == dt and emb.shape == (dim, N) and emb.stride(1) == 1 and emb.stride(0) % 64 == 0
    assert float(emb.float().abs().sum()) == 0.0
    rows = torch.tensor(exp["embeddings"], device=DEV).t().contiguous()                # [N, dim] as encode_corpus returns it
    idx.embeddings[:, 0:4] = rows[0:4].T.to(dt)                                        # rag/eval.py:145
    idx.embeddings[:, 4:] = rows[4:].T.to(dt)
    assert idx.embeddings.data_ptr() == emb.data_ptr() and torch.equal(idx.embeddings, rows.T.to(dt))
    idx.save_index(str(tmp_path), 2)
    back = rag.DistributedIndex(dtype=dt)
    back.load_index(str(tmp_path), 2)
    assert torch.equal(back.embeddings, idx.embeddings) and back.doc_map == idx.doc_map
    assert back.embeddings.shape == (dim, N) and back.embeddings.stride(0) % 64 == 0 and back.embeddings.dtype == dt
    assert torch.load(tmp_path / "embeddings.0.pt").is_contiguous()                   # the files hold plain column blocks
    q = np.asarray(exp["queries"], np.float32)
    e64 = idx.embeddings.double().cpu().numpy()
    col = {json.dumps(p, sort_keys=True): i for i, p in enumerate(passages)}
    for index in (idx, back):
        docs, scores = index.search_knn(torch.from_numpy(q).to(DEV), exp["topk"])
        ix = np.array([[col[json.dumps(d, sort_keys=True)] for d in row] for row in docs])
        _condition4(np.array(scores, np.float32), ix, q, e64, exp["topk"], "DistributedIndex")
        assert not hasattr(index, "_emb32")


def test_search_footprint_is_the_workspace_not_the_index():
    """a bf16 index of 102 MB: the search may allocate its workspace, the queries' fp32 copy and the results -- the route through an
    fp32 copy and a [Q, N] score matrix took twice the index's bytes"""
    from gritlm_amd import _lib, rag
    H, N, Q, k = 256, 200000, 64, 10
    idx = rag.DistributedIndex(dtype=torch.bfloat16)
    idx.init_embeddings([None] * N, H)
    g = torch.Generator(device=DEV).manual_seed(17)
    idx.embeddings[:, :] = torch.randn((H, N), generator=g, device=DEV).to(torch.bfloat16)
    q = torch.randn((Q, H), generator=g, device=DEV)
    index_bytes = H * N * 2
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    docs, scores = idx.search_knn(q, k)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    ws = _lib.load().grit_knn16_workspace_bytes(Q, N, H, k)
    print(f"knn16 footprint: rise {rise} B, workspace {ws} B, index {index_bytes} B")
    assert len(docs) == Q and len(scores[0]) == k and ws > 0
    assert rise <= ws + Q * H * 4 + (1 << 20)
    assert rise < index_bytes / 4
    assert not hasattr(idx, "_emb32")
