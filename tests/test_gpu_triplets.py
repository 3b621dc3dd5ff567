"""The triplet lists of a directed graph built on the device (functional.triplets over dd_csr_select_*), the SparseTensor
facade on the same kernels and the dispatcher op, against ``oracle.ops.bond_triplets`` / plain torch on the CPU copy of the
same input.  Integer lists: compared with ``torch.equal``, no tolerance.  The graphs (tests/triplets_cases.py) are the
smallest at which the kernels can still go wrong: unsorted destinations, nodes without edges, self loops, duplicate edges,
a run longer than a wave and than a block, sizes that are no multiple of 64, and the benchmark's ligand batch."""
import sys

import numpy as np
import pytest
import torch

from decompdiff_amd import functional as F
from decompdiff_amd import hip_lib
import decompdiff_amd.torch_ops as T
import triplets_cases as C
from oracle import ops

pytestmark = pytest.mark.gpu

NAMES = ("i", "j", "idx_i", "idx_j", "idx_k", "idx_kj", "idx_ji")


def _check(ei, n):
    dev = torch.device("cuda:0")
    want = ops.bond_triplets(ei, n)
    got = F.triplets(ei.to(dev), n)
    assert len(got) == 7
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == torch.int64 and g.device.type == "cuda", name
        assert torch.equal(g.cpu(), w), (name, g.numel(), w.numel())
    return got


@pytest.mark.parametrize("name", list(C.CASES))
def test_triplets_match_the_oracle(name):
    build, n_edges, n_triplets = C.CASES[name]
    ei, n = build()
    got = _check(ei, n)
    assert n_edges is None or ei.size(1) == n_edges
    assert n_triplets is None or got[2].numel() == n_triplets
    assert bool((got[6][1:] >= got[6][:-1]).all())                            # idx_ji is sorted by construction


def test_i_and_j_are_the_rows_of_edge_index_and_empty_graphs_need_no_launch():
    dev = torch.device("cuda:0")
    ei = C.scaffold_fc()[0].to(dev)
    got = F.triplets(ei, 5)
    assert got[0].data_ptr() == ei[1].data_ptr() and got[1].data_ptr() == ei[0].data_ptr()
    for n in (1, 0, 7):                                                       # N = 1 with E = 0; no nodes at all
        out = F.triplets(torch.empty(2, 0, dtype=torch.int64, device=dev), n)
        assert len(out) == 7 and all(o.numel() == 0 and o.dtype == torch.int64 and o.is_cuda for o in out)
    # a non-contiguous edge_index (columns of a wider tensor) gives the same lists
    wide = torch.zeros(2, 20, dtype=torch.int64, device=dev)
    wide[:, :14] = ei
    assert all(torch.equal(a, b) for a, b in zip(F.triplets(wide[:, :14], 5), got))


def test_results_are_bit_identical_from_run_to_run():
    ei, n = C.random_graph()
    d = ei.to("cuda:0")
    first = [t.cpu().numpy().tobytes() for t in F.triplets(d, n)]
    for _ in range(19):
        assert [t.cpu().numpy().tobytes() for t in F.triplets(d, n)] == first


def test_dispatcher_op_returns_the_five_lists():
    ei, n = C.two_ligands()
    want = ops.bond_triplets(ei, n)[2:]
    got = torch.ops.decompdiff_amd.triplets(ei.to("cuda:0"), n)
    assert len(got) == 5 and all(torch.equal(g.cpu(), w) for g, w in zip(got, want))
    with pytest.raises(Exception):                                            # CPU tensors: no fallback
        torch.ops.decompdiff_amd.triplets(ei, n)


def _sorted_coo(row, col, value, n_cols):
    perm = torch.argsort(row * n_cols + col, stable=True)
    return row[perm], col[perm], value[perm]


def test_sparse_tensor_method_by_method():
    """The facade against plain torch on the CPU, on the random graph (shuffled COO): the storage triple after construction,
    row selection with repeated and empty rows, set_value(None).sum(dim=1), sparse_sizes; then the whole call site through
    the patched ``torch_sparse`` import."""
    dev = torch.device("cuda:0")
    ei, n = C.random_graph()
    row, col = ei[1], ei[0]                                                   # (the call site's SparseTensor(row=col, col=row))
    value = torch.arange(ei.size(1)) * 3 + 1
    srow, scol, sval = _sorted_coo(row, col, value, n)
    n_rows = n + 2                                                            # (two rows past the graph's: certainly empty)
    t = F.SparseTensor(row=row.to(dev), col=col.to(dev), value=value.to(dev), sparse_sizes=(n_rows, n))
    assert t.sparse_sizes() == (n_rows, n)
    assert torch.equal(t.storage.row().cpu(), srow) and torch.equal(t.storage.col().cpu(), scol) and torch.equal(t.storage.value().cpu(), sval)
    counts = torch.bincount(row, minlength=n_rows)
    empty = (counts == 0).nonzero().flatten().tolist()
    full = (counts > 1).nonzero().flatten().tolist()
    assert empty and full                                                     # rows of both kinds
    index = torch.tensor([full[0], empty[0], full[0], full[-1], n - 1, 0, empty[-1], full[0]])
    sub = t[index.to(dev)]
    want_row = torch.cat([torch.full((int(counts[r]),), p) for p, r in enumerate(index.tolist())])
    want_col = torch.cat([scol[srow == r] for r in index.tolist()])
    want_val = torch.cat([sval[srow == r] for r in index.tolist()])
    assert sub.sparse_sizes() == (index.numel(), n)
    assert torch.equal(sub.storage.row().cpu(), want_row) and torch.equal(sub.storage.col().cpu(), want_col)
    assert torch.equal(sub.storage.value().cpu(), want_val)
    bare = sub.set_value(None)
    assert bare.storage.value() is None and sub.storage.value() is not None
    per_row = bare.sum(dim=1)
    assert per_row.dtype == torch.float32 and torch.equal(per_row.cpu(), counts[index].float())
    none = t[torch.empty(0, dtype=torch.int64, device=dev)]
    assert none.sparse_sizes() == (0, n) and none.storage.row().numel() == 0
    with pytest.raises(IndexError):
        t[torch.tensor([0, n_rows], device=dev)]
    with pytest.raises(IndexError):
        F.SparseTensor(row=torch.tensor([0, n], device=dev), col=torch.tensor([0, 1], device=dev), sparse_sizes=(n, n))
    # the import the reference's encoder makes, and the sequence of calls of its triplets method on that class
    saved = {k: sys.modules.get(k) for k in ("torch_scatter", "torch_cluster", "torch_sparse")}
    try:
        T.patch_reference_imports(force=True)
        import torch_sparse
        assert torch_sparse.SparseTensor is F.SparseTensor
        d = ei.to(dev)
        adj = torch_sparse.SparseTensor(row=d[1], col=d[0], value=torch.arange(d.size(1), device=dev), sparse_sizes=(n, n))
        sel = adj[d[0]]
        num = sel.set_value(None).sum(dim=1).to(torch.long)
        want = ops.bond_triplets(ei, n)
        keep = d[1].repeat_interleave(num) != sel.storage.col()
        assert torch.equal(sel.storage.col()[keep].cpu(), want[4]) and torch.equal(sel.storage.value()[keep].cpu(), want[5])
        assert torch.equal(sel.storage.row()[keep].cpu(), want[6])
    finally:
        for k, m in saved.items():
            if m is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = m


def test_idx_ji_feeds_scatter_attention():
    """Composition on the scaffold_fc-shaped list: idx_ji (sorted, dim_size = E) as the index of functional.scatter_attention
    with random k, v per member and q per edge gathered to the members as the bond layer does, against the oracle's
    scatter_softmax + scatter_sum at the tolerance tests/test_gpu_scatter_ops.py uses for that op (2e-5 absolute, fp64 reference)."""
    dev = torch.device("cuda:0")
    ei, n = C.scaffold_fc()
    E = ei.size(1)
    idx_ji = F.triplets(ei.to(dev), n)[6]
    g = torch.Generator().manual_seed(11)
    M = idx_ji.numel()
    q = torch.randn(E, 128, generator=g)[idx_ji.cpu()]
    k, v = torch.randn(M, 128, generator=g), torch.randn(M, 128, generator=g)
    s = (q.view(-1, 16, 8) * k.view(-1, 16, 8) / np.sqrt(8)).sum(-1)
    alpha = ops.scatter_softmax(s.double(), idx_ji.cpu(), 0, dim_size=E)
    want = ops.scatter_sum(alpha.unsqueeze(-1) * v.view(-1, 16, 8).double(), idx_ji.cpu(), 0, dim_size=E).view(-1, 128)
    got = F.scatter_attention(q.to(dev), k.to(dev), v.to(dev), idx_ji, E).cpu().double()
    assert M == 24 and got.shape == (E, 128)
    assert float((got - want).abs().max()) < 2e-5


def test_errors():
    dev = torch.device("cuda:0")
    ei, n = C.scaffold_fc()
    d = ei.to(dev)
    with pytest.raises(IndexError):
        F.triplets(d, n - 1)                                                  # node id 4 with num_nodes 4
    bad = d.clone()
    bad[0, 3] = -1
    with pytest.raises(IndexError):
        F.triplets(bad, n)
    with pytest.raises(ValueError):
        F.triplets(torch.zeros(3, 14, dtype=torch.int64, device=dev), n)
    with pytest.raises(hip_lib.HipLibraryError):
        F.triplets(ei, n)
    assert len(F.triplets(d, n)[2]) == 24                                     # (the device is fine after the refusals)
