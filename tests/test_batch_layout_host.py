"""decompdiff_amd.batch_layout against brute force written out here: python loops over (b, dst, src), nothing imported from the
module under test (or from synth) for the expected values.  Sizes: a 2-atom ligand (NL - 1 = 1, one bond each way), a repeated
size whose group has two non-adjacent members (0 and 3), a 1-atom pocket."""
import pytest
import torch

from decompdiff_amd import batch_layout as BL

N_P, N_L = [3, 1, 4, 3], [2, 3, 5, 2]
N_B = [n * (n - 1) for n in N_L]


def brute_fc(n, off=0):
    """[(src, dst)] dst-major, sources ascending, of one ligand whose first row is `off`."""
    return [(src + off, dst + off) for dst in range(n) for src in range(n) if src != dst]


def brute_batch(n_l):
    bonds, off = [], 0
    for n in n_l:
        bonds += brute_fc(n, off)
        off += n
    return bonds


def as_index(bonds):
    return torch.tensor(bonds, dtype=torch.long).reshape(-1, 2).t()


def batch_tensors(n_p=N_P, n_l=N_L):
    vec = lambda counts: torch.tensor([b for b, n in enumerate(counts) for _ in range(n)], dtype=torch.long)
    return vec(n_p), vec(n_l), vec([n * (n - 1) for n in n_l]), as_index(brute_batch(n_l))


def layout():
    b_p, b_l, b_b, fc = batch_tensors()
    return BL.BatchLayout.from_batch(b_p, b_l, batch_ligand_bond=b_b, ligand_fc_bond_index=fc, n_bonds=sum(N_B))


def test_fc_bond_index_is_the_dst_major_list():
    for n in (2, 3, 5):
        assert torch.equal(BL.fc_bond_index(n), as_index(brute_fc(n)))
    assert torch.equal(BL.fc_bond_index_batch(N_L), as_index(brute_batch(N_L)))
    assert torch.equal(BL.fc_bond_index_batch([3] * 4), as_index(brute_batch([3, 3, 3, 3])))
    b_p, b_l, fc = BL.dense_vectors(4, 2, 3)
    assert b_p.tolist() == [0, 0, 1, 1, 2, 2, 3, 3] and b_l.tolist() == [b for b in range(4) for _ in range(3)]
    assert torch.equal(fc, as_index(brute_batch([3] * 4)))
    assert BL.batch_vector(4, N_B).tolist() == [b for b, n in enumerate(N_B) for _ in range(n)]


def test_counts_and_density():
    lay = layout()
    assert (lay.B, lay.n_p, lay.n_l, lay.n_b) == (4, N_P, N_L, N_B) and not lay.is_dense
    assert BL.BatchLayout([3, 3], [2, 2]).is_dense and not BL.BatchLayout([3, 3], [2, 3]).is_dense


@pytest.mark.parametrize("NPm,NLm", [(None, None), (8, 8)])
def test_padded_rows(NPm, NLm):
    rows_p, rows_l, rows_b = layout().padded_rows(NPm, NLm)
    NPm, NLm = NPm or max(N_P), NLm or max(N_L)
    Ebm = NLm * (NLm - 1)
    assert rows_p.tolist() == [b * NPm + i for b, n in enumerate(N_P) for i in range(n)]
    assert rows_l.tolist() == [b * NLm + i for b, n in enumerate(N_L) for i in range(n)]
    want = [b * Ebm + dst * (NLm - 1) + (src - (src > dst)) for b, n in enumerate(N_L) for (src, dst) in brute_fc(n)]
    assert rows_b.tolist() == want
    for rows in (rows_p, rows_l, rows_b):
        assert rows.dtype == torch.long and len(set(rows.tolist())) == rows.numel()                  # injective
    # the padded batch's own bond list (dst-major over NLm atoms) has the caller's bond at each of those rows
    padded = brute_batch([NLm] * len(N_L))
    first = [sum(N_L[:b]) for b in range(len(N_L))]
    caller = [(s - first[b] + b * NLm, d - first[b] + b * NLm) for b, n in enumerate(N_L) for (s, d) in brute_fc(n, first[b])]
    assert [padded[r] for r in rows_b.tolist()] == caller


def test_size_groups():
    lay = layout()
    groups = lay.size_groups()
    assert [g.ids for g in groups] == [[0, 3], [1], [2]]
    assert [(g.n_p, g.n_l) for g in groups] == [(3, 2), (1, 3), (4, 5)]
    for rows, total in (("rows_p", sum(N_P)), ("rows_l", sum(N_L)), ("rows_b", sum(N_B))):
        assert sorted(r for g in groups for r in getattr(g, rows).tolist()) == list(range(total))     # a partition
    first_p, first_l, first_b = ([sum(c[:b]) for b in range(4)] for c in (N_P, N_L, N_B))
    fc = as_index(brute_batch(N_L))
    for g in groups:
        assert g.rows_p.tolist() == [first_p[b] + i for b in g.ids for i in range(N_P[b])]
        assert g.rows_l.tolist() == [first_l[b] + i for b in g.ids for i in range(N_L[b])]
        assert g.rows_b.tolist() == [first_b[b] + i for b in g.ids for i in range(N_B[b])]
        # the caller's bonds of the group, renumbered to the group's own rows, are the dense list of its shape
        shift = torch.tensor([k * g.n_l - first_l[b] for k, b in enumerate(g.ids) for _ in range(N_B[b])])
        dense = as_index(brute_batch([g.n_l] * len(g.ids)))
        assert torch.equal(fc[:, g.rows_b] + shift, dense)
        b_p, b_l, fc_g = BL.dense_vectors(len(g.ids), g.n_p, g.n_l)
        assert torch.equal(fc_g, dense) and b_p.numel() == g.rows_p.numel() and b_l.numel() == g.rows_l.numel()
    # keys that differ inside a size split its group; prior / full-protein counts are keys of their own
    assert [g.ids for g in lay.size_groups(extra_keys=[0, 0, 1, 1])] == [[0], [1], [2], [3]]
    assert [g.ids for g in lay.size_groups(extra_keys=[0, 0, 0, 0])] == [[0, 3], [1], [2]]
    pri = BL.BatchLayout(N_P, N_L, n_pr=[3, 3, 3, 2], n_f=[7, 7, 7, 7])
    groups = pri.size_groups()
    assert [g.ids for g in groups] == [[0], [1], [2], [3]]
    assert [g.rows_pr.tolist() for g in groups] == [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10]]
    assert [g.first_pr for g in groups] == [[0], [3], [6], [9]] and groups[3].rows_f.tolist() == list(range(21, 28))


def test_validation():
    b_p, b_l, b_b, fc = batch_tensors()
    with pytest.raises(NotImplementedError, match="dst-major"):
        BL.BatchLayout.from_batch(b_p, b_l, ligand_fc_bond_index=fc.flip(0))
    with pytest.raises(NotImplementedError, match="sorted"):
        BL.BatchLayout.from_batch(b_p, b_l.flip(0), ligand_fc_bond_index=fc)
    with pytest.raises(NotImplementedError, match="sorted"):
        BL.BatchLayout.from_batch(b_p, b_l, batch_prior=torch.tensor([0, 2, 1, 3]))
    perm = b_b.clone()
    perm[0], perm[-1] = b_b[-1], b_b[0]
    with pytest.raises(NotImplementedError, match="batch_ligand_bond"):
        BL.BatchLayout.from_batch(b_p, b_l, batch_ligand_bond=perm, ligand_fc_bond_index=fc)
    with pytest.raises(NotImplementedError, match="dst-major"):
        BL.BatchLayout.from_batch(b_p, b_l, n_bonds=sum(N_B) + 2)
    with pytest.raises(NotImplementedError, match="at least 2 ligand atoms"):
        BL.BatchLayout.from_batch(*batch_tensors(N_P, [2, 1, 5, 2])[:2])
    with pytest.raises(NotImplementedError, match="protein atoms"):
        BL.BatchLayout.from_batch(torch.tensor([0, 0, 2, 3]), b_l)
    with pytest.raises(ValueError, match="empty batch"):
        BL.BatchLayout.from_batch(b_p[:0], b_l)


def test_fits_padded_and_size_limits():
    lay = BL.BatchLayout([40, 30], [10, 4])                                # the smallest sample has 34 atoms
    assert BL.fits_padded(lay, 32) and BL.fits_padded(lay, 33) and not BL.fits_padded(lay, 34)
    assert BL.fits_padded(BL.BatchLayout([3, 4], [2, 3]), 32) is False      # K = min(knn, 7 - 1) = 6 > 5 - 1
    assert BL.fits_padded(BL.BatchLayout([3, 4], [3, 3]), 5) and BL.fits_padded(BL.BatchLayout([3, 4], [3, 3]), 5, 32, 4)
    big = BL.BatchLayout([1990, 40], [40, 100])                           # each sample fits, the padded shape (2090) does not
    assert not BL.fits_padded(big, 32) and BL.fits_padded(big, 32, size_limits=False)
    assert not BL.fits_padded(BL.BatchLayout([40, 40], [129, 40]), 32)
    BL.check_size_limits(1920, 128)
    BL.check_size_limits([1990, 40], [40, 100])
    for n_p, n_l in ((40, 129), (40, 1), (2008, 41), ([40, 40], [40, 129]), ([2040, 40], [9, 9])):
        with pytest.raises(NotImplementedError):
            BL.check_size_limits(n_p, n_l)
