"""Host-side bookkeeping of a flat PyG-style batch (sorted batch vectors, one dst-major fully connected bond list per ligand):
the bond lists, the per-sample counts and their validation, the row maps into the padded dense layout, the groups of samples
of equal size, and the limits of the padded path.  model.py and training.py build none of this themselves."""
from __future__ import annotations

from dataclasses import dataclass
from itertools import accumulate
from typing import List, Optional, Sequence

import numpy as np
import torch

NL_MIN, NL_MAX, N_MAX = 2, 128, 2048      # ligand atoms / atoms per sample the kernels take (include/: DD_NL_MAX, DD_N_MAX)

_FC_ERROR = "ligand_fc_bond_index must be the dst-major fully connected graph ('fc' mode)"


def fc_bond_index(n: int, device=None) -> torch.Tensor:
    """[2, n (n - 1)] (src, dst) of FeaturizeLigandBond('fc') (utils/transforms.py:331-337): dst-major, sources ascending.
    Bond (src -> dst) is row dst * (n - 1) + sp with sp = src - (src > dst), the source's position among the n - 1 others."""
    dst = torch.arange(n, device=device).repeat_interleave(max(n - 1, 0))
    sp = torch.arange(max(n - 1, 0), device=device).repeat(n)
    return torch.stack([sp + (sp >= dst), dst], 0)


def fc_bond_index_batch(n_l: Sequence[int], device=None) -> torch.Tensor:
    """The bond lists of ligands of n_l[b] atoms, each offset by its first ligand row (PyG collate, utils/data.py:443-444);
    ``[NL] * B`` gives the list of a dense batch."""
    one = {n: fc_bond_index(n, device) for n in set(n_l)}
    return torch.cat([one[n] + o for n, o in zip(n_l, accumulate(n_l, initial=0))], 1)


def batch_vector(B: int, counts, device=None) -> torch.Tensor:
    """PyG batch vector: sample b repeated counts[b] times (an int: the same count for all -- no host data, capturable)."""
    ids = torch.arange(B, device=device)
    if isinstance(counts, int):
        return ids.repeat_interleave(counts)
    return ids.repeat_interleave(torch.tensor(counts, device=device), output_size=sum(counts))


def dense_vectors(B: int, NP: int, NL: int, device=None):
    """(batch_protein, batch_ligand, ligand_fc_bond_index) of a dense batch of B samples with NP + NL atoms each."""
    return batch_vector(B, NP, device), batch_vector(B, NL, device), fc_bond_index_batch([NL] * B, device)


def sample_counts(batch: torch.Tensor, B: int = 0, name: Optional[str] = None) -> List[int]:
    """Rows per sample of a batch vector (one device -> host copy); with ``name``, first the check that it is sorted."""
    if name is not None and batch.numel() > 1 and bool((batch[1:] < batch[:-1]).any().item()):
        raise NotImplementedError(f"{name} must be sorted (PyG Batch order)")
    return torch.bincount(batch, minlength=B).tolist()


def block_rows(counts: Sequence[int], width: int) -> torch.Tensor:
    """Flat row -> row of a [B * width] array in which sample b's rows are the first counts[b] of its block (host)."""
    return torch.from_numpy(np.concatenate([np.arange(b * width, b * width + n) for b, n in enumerate(counts)]))


def check_size_limits(n_p, n_l):
    """Raise for sizes (ints, or per-sample lists) outside what the kernels take."""
    n_p, n_l = ([n_p], [n_l]) if isinstance(n_l, int) else (n_p, n_l)
    for n in n_l:
        if not NL_MIN <= n <= NL_MAX:
            raise NotImplementedError(f"ligand size {n} outside the supported range [{NL_MIN}, {NL_MAX}]")
    if max(a + b for a, b in zip(n_p, n_l)) > N_MAX:
        raise NotImplementedError(f"more than {N_MAX} atoms per sample")


@dataclass
class SizeGroup:
    """Samples ``ids`` of one size and their flat rows (host index tensors, samples in ascending order).  Its dense batch
    vectors and bond index are `dense_vectors(len(ids), n_p, n_l)`: what the validated bond list becomes once renumbered."""
    ids: List[int]
    n_p: int
    n_l: int
    n_pr: int
    n_f: int
    rows_p: torch.Tensor
    rows_l: torch.Tensor
    rows_b: torch.Tensor
    rows_pr: torch.Tensor
    rows_f: torch.Tensor
    first_pr: List[int]                       # first prior row of every member (to renumber indices into the prior rows)


class BatchLayout:
    """Per-sample row counts of a batch -- protein n_p, ligand n_l, bonds n_b = n_l (n_l - 1), prior n_pr and full-protein
    n_f (zeros if absent) -- and everything that follows from them.  `from_batch` counts and validates a caller's tensors;
    the constructor takes counts that are already established."""

    def __init__(self, n_p, n_l, n_pr=None, n_f=None):
        self.n_p, self.n_l, self.B = list(n_p), list(n_l), len(n_p)
        self.n_pr = list(n_pr) if n_pr is not None else [0] * self.B
        self.n_f = list(n_f) if n_f is not None else [0] * self.B
        self.n_b = [n * (n - 1) for n in self.n_l]
        self.is_dense = len(set(zip(self.n_p, self.n_l))) == 1

    @classmethod
    def from_batch(cls, batch_protein, batch_ligand, batch_prior=None, full_batch_protein=None, batch_ligand_bond=None,
                   ligand_fc_bond_index=None, n_bonds=None, need_protein=True) -> "BatchLayout":
        """Sorted batch vectors -> counts (one bincount per vector); every ligand has at least 2 atoms; the bond list, the bond
        batch vector and the bond count (each if given) are those of the per-sample dst-major fully connected graphs."""
        if batch_protein.numel() == 0 or batch_ligand.numel() == 0:
            raise ValueError("empty batch")
        n_p = sample_counts(batch_protein, 0, "batch_protein")
        B = len(n_p)
        n_l = sample_counts(batch_ligand, B, "batch_ligand")
        if len(n_l) != B or min(n_l) < NL_MIN or (need_protein and min(n_p) < 1):
            raise NotImplementedError("every sample needs protein atoms and at least 2 ligand atoms")
        lay = cls(n_p, n_l, None if batch_prior is None else sample_counts(batch_prior, B, "batch_prior"),
                  None if full_batch_protein is None else sample_counts(full_batch_protein, B))
        fc, blb = ligand_fc_bond_index, batch_ligand_bond
        if n_bonds is not None and n_bonds != sum(lay.n_b):
            raise NotImplementedError(_FC_ERROR)
        if fc is not None and (tuple(fc.shape) != (2, sum(lay.n_b)) or not torch.equal(fc, fc_bond_index_batch(n_l, fc.device))):
            raise NotImplementedError(_FC_ERROR)
        if blb is not None and (blb.numel() != sum(lay.n_b) or not torch.equal(blb, batch_vector(B, lay.n_b, blb.device))):
            raise NotImplementedError("batch_ligand_bond does not match the fully connected bond lists")
        return lay

    def padded_rows(self, NPm=None, NLm=None):
        """(rows_p, rows_l, rows_b), host: flat protein / ligand / bond row -> row of the padded [B*NPm] / [B*NLm] /
        [B*NLm(NLm-1)] arrays (default: the batch maxima), whose sample blocks start with the real atoms and hold the dst-major
        bond list over NLm atoms."""
        NPm, NLm = NPm or max(self.n_p), NLm or max(self.n_l)
        one = {}
        for n in set(self.n_l):
            src, dst = fc_bond_index(n).numpy()
            one[n] = dst * (NLm - 1) + (src - (src > dst))
        rows_b = np.concatenate([b * NLm * (NLm - 1) + one[n] for b, n in enumerate(self.n_l)])
        return block_rows(self.n_p, NPm), block_rows(self.n_l, NLm), torch.from_numpy(rows_b)

    def size_groups(self, extra_keys=()) -> List[SizeGroup]:
        """The samples grouped by (n_p, n_l, n_pr, n_f) and, if given, extra_keys[b]; groups in order of their first member."""
        members = {}
        for b in range(self.B):
            members.setdefault((self.n_p[b], self.n_l[b], self.n_pr[b], self.n_f[b], extra_keys[b] if extra_keys else None), []).append(b)
        counts = (self.n_p, self.n_l, self.n_b, self.n_pr, self.n_f)
        offs = [list(accumulate(c, initial=0)) for c in counts]
        rng = lambda o, c, ids: torch.from_numpy(np.concatenate([np.arange(o[b], o[b] + c[b]) for b in ids]))
        return [SizeGroup(ids, key[0], key[1], key[2], key[3], *(rng(o, c, ids) for o, c in zip(offs, counts)),
                          first_pr=[offs[3][b] for b in ids]) for key, ids in members.items()]


def fits_padded(layout: BatchLayout, knn: int, NPm=None, NLm=None, size_limits=True) -> bool:
    """Can the batch run as ONE dense pass padded to NPm + NLm atoms per sample (default: the batch maxima)?  Every sample
    needs K + 1 real atoms, K the kNN degree of the padded shape (its lists would be shorter than the others' otherwise);
    ``size_limits``: and the padded shape must be one the fused kernels take."""
    NPm, NLm = NPm or max(layout.n_p), NLm or max(layout.n_l)
    if min(a + b for a, b in zip(layout.n_p, layout.n_l)) < min(int(knn), NPm + NLm - 1) + 1:
        return False
    return not size_limits or (min(layout.n_l) >= NL_MIN and NLm <= NL_MAX and NPm + NLm <= N_MAX)
