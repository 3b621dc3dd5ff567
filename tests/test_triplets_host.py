"""The triplet lists of the ligand bond graph at the op level (functional.triplets, functional.SparseTensor,
torch.ops.decompdiff_amd.triplets, the C-ABI family dd_csr_select_*): everything that can be checked without a GPU -- the
public names and signatures, header / binding / library agreement, the host-side argument checks of the entry points (they
return before any launch), the exceptions of the Python surface, and the op's schema and fake implementation."""
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch

from decompdiff_amd import functional as F
from decompdiff_amd import hip_lib
import decompdiff_amd.torch_ops as T
import triplets_cases as C
from oracle import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dd_csr_select_scratch_bytes", "dd_csr_select_count", "dd_csr_select_fill")


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    return hip_lib.load()


def test_public_names_and_signatures():
    assert list(inspect.signature(F.triplets).parameters) == ["edge_index", "num_nodes"]
    assert list(inspect.signature(F.SparseTensor.__init__).parameters)[1:5] == ["row", "col", "value", "sparse_sizes"]
    for name in ("__getitem__", "set_value", "sum", "sparse_sizes"):
        assert callable(getattr(F.SparseTensor, name)), name
    assert "capture" in F.triplets.__doc__                                  # (the host read per call is documented)
    schema = str(torch.ops.decompdiff_amd.triplets.default._schema)
    assert schema == "decompdiff_amd::triplets(Tensor edge_index, SymInt num_nodes) -> (Tensor, Tensor, Tensor, Tensor, Tensor)", schema


def test_entry_points_are_declared_bound_and_exported():
    lib = _lib()
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "decompdiff_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert name in hip_lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    assert lib.dd_csr_select_scratch_bytes.restype is ctypes.c_size_t
    assert lib.dd_abi_version() == 9                                         # additive: the ABI version stays


def test_entry_points_check_their_arguments_before_any_launch():
    lib = _lib()
    size = lib.dd_csr_select_scratch_bytes
    # header (total, bad) + deg[N] + ptr[N+1] + two 64-bit words per entry + off[R+1] + skip_lb[R], every part padded to 8 bytes
    assert size(0, 0, 0, 0) == 16 + 0 + 8 + 0 + 8 + 0
    assert size(14, 5, 5, 14) == 16 + 24 + 24 + 2 * 8 * 14 + 64 + 56
    assert size(6960, 2640, 2640, 6960) > size(6960, 2640, 2640, 0) > size(0, 2640, 2640, 0)
    big = 1 << 31
    for args in ((big, 1, 1, 1), (1, big, 1, 1), (1, 1, big, 1), (1, 1, 1, big), (-1, 1, 1, 1), (1, 1, 1, -1)):
        assert size(*args) == 0, args
    assert size(big - 1, 1, 1, 1) > 16 * (big - 1)                           # (size_t: no 32-bit wrap)
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 8)
    count, fill = lib.dd_csr_select_count, lib.dd_csr_select_fill
    assert count(p, p, 4, 3, 3, p, None, 4, None, 1 << 20, None) == -1       # no scratch
    assert count(p, p, 4, 3, 3, p, None, 4, ctypes.c_void_p(p.value + 4), 1 << 20, None) == -1   # scratch not 8-byte aligned
    assert count(None, p, 4, 3, 3, p, None, 4, p, 1 << 20, None) == -1       # entries without their arrays
    assert count(p, p, 4, 3, 3, None, None, 4, p, 1 << 20, None) == -1       # a selection without its array
    assert count(p, p, -1, 3, 3, p, None, 4, p, 1 << 20, None) == -1
    assert count(p, p, big, 3, 3, p, None, 4, p, 1 << 20, None) == -2        # int32 inside: refused, not wrapped
    assert count(p, p, 4, 3, 3, p, None, big, p, 1 << 20, None) == -2
    assert count(p, p, 4, 3, 3, p, None, 4, p, size(4, 3, 3, 4) - 1, None) == -3
    assert fill(p, None, 4, 3, 3, 4, p, big, p, p, p, None, None, None) == -2      # a total at or above 2^31
    assert fill(p, None, 4, 3, 3, 4, p, -1, p, p, p, None, None, None) == -1
    assert fill(p, None, 4, 3, 3, 4, p, 0, p, p, p, None, None, None) == 0         # nothing to write: no launch
    assert fill(p, None, 4, 3, 3, 4, None, 5, p, p, p, None, None, None) == -1     # no scratch
    assert fill(p, None, 4, 3, 3, 4, p, 5, p, p, p, None, p, None) == -1           # out_skip without skip


def test_cpu_tensors_raise_and_bad_shapes_are_value_errors():
    ei, n = C.scaffold_fc()
    with pytest.raises(hip_lib.HipLibraryError):
        F.triplets(ei, n)                                                     # no CPU implementation
    with pytest.raises(hip_lib.HipLibraryError):
        F.SparseTensor(row=ei[1], col=ei[0], value=torch.arange(ei.size(1)), sparse_sizes=(n, n))
    for bad in (torch.zeros(3, 14, dtype=torch.int64), ei.to(torch.int32), ei[0], ei.t().contiguous(), ei.double()):
        with pytest.raises(ValueError):
            F.triplets(bad, n)
    with pytest.raises(ValueError):
        F.triplets(ei, -1)
    with pytest.raises(ValueError):
        F.SparseTensor(row=ei[1].to(torch.int32), col=ei[0], sparse_sizes=(n, n))
    with pytest.raises(ValueError):
        F.SparseTensor(row=ei[1], col=ei[0, :3], sparse_sizes=(n, n))
    with pytest.raises(NotImplementedError):
        F.SparseTensor(row=ei[1], col=ei[0])                                  # sparse_sizes is what the call site gives


def test_sparse_tensor_refuses_what_the_call_site_does_not_touch():
    t = F.SparseTensor._sorted(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), None, (4, 4))
    assert t.sparse_sizes() == (4, 4) and t.storage.value() is None
    for call in (lambda: t.to_dense(), lambda: t.t(), lambda: t.coo(), lambda: t.set_value(torch.zeros(0)), lambda: t.sum(dim=0),
                 lambda: t.sum(), lambda: t[0], lambda: t[torch.zeros(2, dtype=torch.bool)]):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(NotImplementedError, match="to_dense"):
        t.to_dense()
    assert not hasattr(t, "__array__")                                        # (protocol lookups stay AttributeError)


def test_patch_installs_torch_sparse_only_where_it_is_missing(monkeypatch):
    for name in ("torch_scatter", "torch_cluster", "torch_sparse"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    real = type(sys)("torch_sparse")
    monkeypatch.setitem(sys.modules, "torch_sparse", real)
    T.patch_reference_imports()
    assert sys.modules["torch_sparse"] is real                                # an importable package is left alone ...
    assert sys.modules["torch_scatter"].scatter_sum and sys.modules["torch_cluster"].knn_graph   # (unchanged behaviour)
    T.patch_reference_imports(force=True)                                     # ... unless forced
    import torch_sparse
    assert torch_sparse.SparseTensor is F.SparseTensor
    monkeypatch.delitem(sys.modules, "torch_sparse")
    try:
        import torch_sparse as installed                                      # noqa: F401
    except ImportError:
        monkeypatch.delitem(sys.modules, "torch_sparse", raising=False)
        T.patch_reference_imports()                                           # not importable: installed without force
        assert sys.modules["torch_sparse"].SparseTensor is F.SparseTensor
    for name in ("torch_scatter", "torch_cluster", "torch_sparse"):
        monkeypatch.delitem(sys.modules, name, raising=False)


def test_op_has_a_fake_implementation_with_one_data_dependent_length():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.symbolic_shapes import ShapeEnv
    with FakeTensorMode(shape_env=ShapeEnv()):
        ei = torch.empty(2, 14, dtype=torch.int64)
        out = torch.ops.decompdiff_amd.triplets(ei, 5)
    assert len(out) == 5 and all(o.dtype == torch.int64 and o.dim() == 1 for o in out)
    n = out[0].shape[0]
    assert isinstance(n, torch.SymInt) and not isinstance(n, int)             # unbacked: known only when the kernels have run
    assert all(o.shape[0] is n or str(o.shape[0]) == str(n) for o in out)     # the five lists share it


def test_cases_have_the_sizes_they_are_named_for():
    """The graphs of the GPU tests, on the oracle: edge and triplet counts as stated, idx_ji non-decreasing."""
    for name, (build, n_edges, n_triplets) in C.CASES.items():
        ei, n = build()
        got = ops.bond_triplets(ei, n)
        assert n_edges is None or ei.size(1) == n_edges, name
        assert n_triplets is None or got[2].numel() == n_triplets, name
        assert bool((got[6][1:] >= got[6][:-1]).all()), name
    ei, _ = C.scaffold_fc()
    assert bool((ei[1, 1:] < ei[1, :-1]).any())                               # destinations not sorted
    assert C.random_graph()[0].size(1) % 64 != 0 and C.hub()[0].size(1) % 64 != 0
