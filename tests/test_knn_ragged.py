"""kNN graphs over a flat, ragged batch (a PyG ``Batch`` of different complexes): the C-ABI entry ``dd_knn_csr``, the drop-in
``functional.knn_graph`` and the registered op ``torch.ops.decompdiff_amd.knn_graph``.

The GPU cases compare the whole ``edge_index`` with a brute-force kNN written here, with ``torch.equal`` (no tolerance): per
sample on the CPU in fp32, ``d2 = (dx*dx + dy*dy) + dz*dz`` by separate torch ops (no FMA), a stable sort by ``(d2, index)``,
the first ``k_b = min(k, n_b - 1)`` (``loop``: ``min(k, n_b)``) neighbours of every centre.  One reference per input is
computed once and shared by the cases that use it."""
import ctypes
import os
import re

import pytest
import torch

from decompdiff_amd import functional, hip_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 32, 33, 64)


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------ CPU
def test_dd_knn_csr_exported_and_declared():
    import __graft_entry__
    __graft_entry__.build()
    lib = hip_lib.load()
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "decompdiff_hip.h")).read(), flags=re.S)
    assert "dd_knn_csr" in hip_lib.EXPORTED_SYMBOLS and hasattr(lib, "dd_knn_csr") and re.search(r"\bdd_knn_csr\s*\(", hdr)
    assert lib.dd_abi_version() == hip_lib.ABI_VERSION == 9               # additive entry point
    # bad arguments are refused before anything touches a device pointer; an empty problem launches nothing
    assert lib.dd_knn_csr(None, None, 1, 4, 4, 3, 0, None, 0, None, None) == -1
    one = (ctypes.c_int64 * 2)()
    p = ctypes.cast(one, ctypes.c_void_p)
    assert lib.dd_knn_csr(None, p, 1, 4, 4, 65, 0, p, 0, None, None) == -2   # K beyond DD_KNN_MAX
    assert lib.dd_knn_csr(None, p, 1, 4, 4, 3, 2, p, 0, None, None) == -1    # loop is 0 or 1
    assert lib.dd_knn_csr(None, p, 1, 0, 0, 3, 0, p, 0, None, None) == 0     # no rows
    assert lib.dd_knn_csr(None, p, 1, 1, 1, 3, 0, p, 0, None, None) == 0     # no edges


def test_knn_graph_argument_checks_need_no_device():
    x = torch.randn(10, 3)
    with pytest.raises(ValueError):
        functional.knn_graph(x, 4, flow="sideways")
    with pytest.raises(hip_lib.HipLibraryError):                           # CPU tensors: no fallback, ragged or not
        functional.knn_graph(x, 4, torch.tensor([0] * 3 + [1] * 7), loop=True)


# ------------------------------------------------------------------------------------ reference
def _orders(x, batch, loop):
    """Per sample (rows, order): order[c] = the sample's rows in ascending (d2, index) seen from centre c, self excluded unless
    `loop`, cut to the 64 nearest.  CPU tensors x [n,3] fp32 / batch [n] (sorted)."""
    out = []
    for b in torch.unique_consecutive(batch).tolist():
        rows = (batch == b).nonzero().squeeze(1)
        xs = x[rows]
        nb = rows.numel()
        dx = xs[:, None, 0] - xs[None, :, 0]
        dy = xs[:, None, 1] - xs[None, :, 1]
        dz = xs[:, None, 2] - xs[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz                                  # [centre, candidate], separate fp32 ops (no FMA)
        order = torch.sort(d2, dim=1, stable=True).indices                  # ascending (d2, index)
        if not loop:                                                        # drop the centre from its own row, order kept
            keep = order != torch.arange(nb)[:, None]
            order = order[keep].view(nb, nb - 1)
        out.append((rows, order[:, :64].clone()))
    return out


def brute_force(orders, k, loop):
    """edge_index [2,E] (row 0 neighbour, row 1 centre): the first k_b = min(k, n_b - 1) (loop: min(k, n_b)) of every row."""
    src, dst = [], []
    for rows, order in orders:
        kb = min(k, order.size(1))
        if kb <= 0:
            continue
        src.append(rows[order[:, :kb]].reshape(-1))
        dst.append(rows.repeat_interleave(kb))
    if not src:
        return torch.empty(2, 0, dtype=torch.long)
    return torch.stack([torch.cat(src), torch.cat(dst)], 0)


def _points(counts, seed, duplicates=False):
    g = torch.Generator().manual_seed(seed)
    n = sum(counts)
    x = torch.randn(n, 3, generator=g) * 6.0
    if duplicates:                                       # coordinates on a coarse lattice: many equal distances, and exact copies
        x = torch.round(x)
        x[5::7] = x[2]
    ids = [i for i, _ in enumerate(counts)]
    batch = torch.cat([torch.full((c,), i, dtype=torch.long) for i, c in zip(ids, counts)])
    return x, batch


# sizes: 1, 2, fewer than k + 1 atoms, the wave width (63-65), a pocket + ligand (347 + 37), an empty id (0), and samples beyond
# one chunk of 2048 candidates (2500: two chunks, 4100: three, the last one 4 candidates long)
MIXED = [1, 2, 0, 20, 63, 64, 65, 384, 2500, 33, 4100, 5]
SMALL = [40, 1, 70, 0, 0, 129, 2]                        # largest sample 129: the 4-candidates-per-lane kernel
_CACHE = {}


def case(name):
    """(x, batch on the CPU, {loop: per-sample sorted orders}) of a named input, built once."""
    if name not in _CACHE:
        if name == "mixed":
            x, batch = _points(MIXED, 1)
        elif name == "small_ties":
            x, batch = _points(SMALL, 2, duplicates=True)
        elif name == "ties_chunked":                     # duplicated points in a sample longer than a chunk of its kernel
            x, batch = _points([300, 2200], 3, duplicates=True)
        elif name == "single":
            x, batch = _points([2300], 4)
            batch = None
        _CACHE[name] = (x, batch, {})
    return _CACHE[name]


def want(name, k, loop=False):
    x, batch, refs = case(name)
    if loop not in refs:                                  # the sort is shared by every k
        refs[loop] = _orders(x, torch.zeros(x.size(0), dtype=torch.long) if batch is None else batch, loop)
    return brute_force(refs[loop], k, loop)


def got(name, k, loop=False, flow="source_to_target", fn=None):
    x, batch, _ = case(name)
    fn = fn or functional.knn_graph
    out = fn(x.to(dev()), k, None if batch is None else batch.to(dev()), loop, flow)
    assert out.dtype == torch.long and out.is_cuda
    return out.cpu()


# ------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_ragged_knn_equals_brute_force(k):
    """Counts 1, 2, < k + 1, 63-65, 384, an id missing from `batch`, 2500 and 4100 (chunked path and its carry)."""
    e = got("mixed", k)
    w = want("mixed", k)
    print(f"k={k}: {e.size(1)} edges over samples of {MIXED}")
    assert e.shape == w.shape and torch.equal(e, w)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["small_ties", "ties_chunked"])
def test_ragged_knn_ties_resolved_by_index(name, k):
    """Lattice coordinates with exact copies of a point: equal d2 everywhere, inside a chunk and across the carry."""
    e, w = got(name, k), want(name, k)
    assert e.shape == w.shape and torch.equal(e, w)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_ragged_knn_loop_and_flow(k):
    w = want("small_ties", k, loop=True)
    e = got("small_ties", k, loop=True)
    assert e.shape == w.shape and torch.equal(e, w)
    assert torch.equal(got("small_ties", k, loop=True, flow="target_to_source"), w.flip(0))
    assert torch.equal(got("small_ties", k, flow="target_to_source"), want("small_ties", k).flip(0))
    if k == 33:                                           # loop across the chunk carry: the centre of row 2100 lives in chunk 2
        assert torch.equal(got("ties_chunked", k, loop=True), want("ties_chunked", k, loop=True))


@pytest.mark.gpu
@pytest.mark.parametrize("k", (1, 64))
def test_knn_without_batch_beyond_one_chunk(k):
    """batch=None with 2300 rows: one sample, beyond the dense kernel's 2048 atoms."""
    e, w = got("single", k), want("single", k)
    assert e.shape == (2, 2300 * k) and torch.equal(e, w)


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,k", [(3, 70, 32), (2, 384, 48), (1, 2048, 64), (4, 9, 33)])
def test_dense_batch_through_the_new_entry_equals_the_dense_path(B, N, k):
    """Equal counts keep dd_knn; the same input pushed through dd_knn_csr gives the same edge_index."""
    x = torch.randn(B * N, 3, generator=torch.Generator().manual_seed(7)).to(dev()) * 5.0
    batch = torch.arange(B, device=dev()).repeat_interleave(N)
    dense = functional.knn_graph(x, k, batch)
    csr = functional._knn_graph_csr(x.contiguous(), k, batch, B, False)
    assert dense.shape == (2, B * N * min(k, N - 1)) and torch.equal(dense, csr)
    if B == 3:                                            # ... and through the ctypes binding of the same entry
        state = dict(functional._ext_state)
        functional._ext_state.update(tried=True, ops=None)
        try:
            assert torch.equal(functional._knn_graph_csr(x.contiguous(), k, batch, B, False), dense)
        finally:
            functional._ext_state.update(state)


@pytest.mark.gpu
@pytest.mark.parametrize("n_max", (1, 129, 300, 5000))
def test_chunk_size_hint_does_not_change_the_result(n_max):
    """dd_knn_csr's n_max only picks the candidates per lane: 1 streams the 129-row sample in two 128-row chunks of the
    smallest kernel, 5000 runs everything in one chunk of the largest."""
    x, batch, _ = case("small_ties")
    k, B, n = 33, len(SMALL), x.size(0)
    counts = torch.tensor(SMALL)
    ptr = torch.zeros(B + 1, dtype=torch.int32)
    ptr[1:] = counts.cumsum(0)
    off = torch.zeros(B + 1, dtype=torch.int64)
    off[1:] = (counts * (counts - 1).clamp(min=0, max=k)).cumsum(0)
    E = int(off[-1])
    xd, pd, od = x.to(dev()).contiguous(), ptr.to(dev()), off.to(dev())
    out = torch.full((2, E), -1, dtype=torch.int64, device=dev())
    hip_lib.check(hip_lib.load().dd_knn_csr(hip_lib.ptr(xd), hip_lib.ptr(pd), B, n, n_max, k, 0, hip_lib.ptr(od), E, hip_lib.ptr(out),
                                            hip_lib.stream_ptr()), "dd_knn_csr")
    assert torch.equal(out.cpu(), want("small_ties", k))


@pytest.mark.gpu
def test_registered_op_follows_the_functional_call():
    import decompdiff_amd.torch_ops  # noqa: F401  (registers torch.ops.decompdiff_amd.*)
    op = torch.ops.decompdiff_amd.knn_graph
    w = want("small_ties", 33)
    assert torch.equal(got("small_ties", 33, fn=op), w)
    assert torch.equal(got("small_ties", 33, fn=functional.knn_graph), w)
    assert torch.equal(got("small_ties", 32, loop=True, flow="target_to_source", fn=op), want("small_ties", 32, loop=True).flip(0))


@pytest.mark.gpu
def test_unsorted_batch_still_raises():
    x = torch.randn(12, 3, device=dev())
    with pytest.raises(NotImplementedError):
        functional.knn_graph(x, 3, torch.tensor([0] * 5 + [2] * 3 + [1] * 4, device=dev()))
