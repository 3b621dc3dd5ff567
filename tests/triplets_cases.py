"""Graphs for the triplet-list tests (functional.triplets / dd_csr_select_*): the smallest ones at which the kernels can still
go wrong, built on the CPU.  Each builder returns ``(edge_index [2,E] int64, num_nodes)``; edge ``e`` is
``edge_index[0, e] -> edge_index[1, e]`` (j -> i).  The expected lists come from ``oracle.ops.bond_triplets``."""
import torch


def _edges(pairs):
    return torch.tensor(pairs, dtype=torch.int64).reshape(-1, 2).t().contiguous()


def fully_connected(ids):
    """Dst-major fully connected list on the given node ids (the ligand bond list of the fused sampler)."""
    return [(s, d) for d in ids for s in ids if s != d]


def fc(n_atoms):
    return _edges(fully_connected(range(n_atoms))), n_atoms


def bench_ligands(n_atoms=30, batch=8, n_protein=300):
    """`batch` ligands of `n_atoms` atoms at node ids (n_protein + n_atoms) * b + n_protein ... (the benchmark's layout)."""
    per = n_protein + n_atoms
    pairs = [p for b in range(batch) for p in fully_connected(range(per * b + n_protein, per * (b + 1)))]
    return _edges(pairs), per * batch


def two_ligands():
    """Fully connected on ids 7..11 and 20..22 within 30 nodes: nodes without edges before, between and after."""
    return _edges(fully_connected(range(7, 12)) + fully_connected(range(20, 23))), 30


def scaffold_fc():
    """A fully connected arm {0, 1, 2}, then the edges from the scaffold atoms {3, 4} to every atom: destinations not sorted."""
    return _edges(fully_connected(range(3)) + [(s, d) for s in (3, 4) for d in range(5) if s != d]), 5


def decomp_fc():
    """Fully connected within groups of 1, 2 and 5 atoms (the group of one contributes no edge)."""
    return _edges(fully_connected([0]) + fully_connected([1, 2]) + fully_connected(range(3, 8))), 8


def random_graph(self_loops=False, duplicates=False, n=12, density=0.35, seed=7):
    """A simple directed graph without i -> j => j -> i symmetry, its edge order shuffled; optionally two self loops, or five
    of its edges repeated (appended, then shuffled with the rest)."""
    g = torch.Generator().manual_seed(seed)
    adj = torch.rand(n, n, generator=g) < density
    adj.fill_diagonal_(False)
    pairs = adj.nonzero().tolist()                                   # (src, dst)
    assert any(not adj[d, s] for s, d in pairs)
    if self_loops:
        pairs += [(3, 3), (8, 8)]
    if duplicates:
        pairs += [pairs[p] for p in (0, 5, 11, 17, 23)]
    order = torch.randperm(len(pairs), generator=g).tolist()
    return _edges([pairs[p] for p in order]), n


def hub():
    """257 edges into node 0 and 3 edges out of it (to two of its sources and to a node without other edges): a run longer than
    a wave and longer than 256; E = 260 is no multiple of 64."""
    return _edges([(k, 0) for k in range(1, 258)] + [(0, 1), (0, 2), (0, 299)]), 300


# name -> (builder, edges, triplets)
CASES = {
    "fc2": (lambda: fc(2), 2, 0),
    "fc3": (lambda: fc(3), 6, 6),
    "fc4": (lambda: fc(4), 12, 24),
    "bench_30x8": (bench_ligands, 6960, 194880),
    "two_ligands": (two_ligands, 26, 66),
    "scaffold_fc": (scaffold_fc, 14, 24),
    "decomp_fc": (decomp_fc, 22, None),
    "random": (random_graph, None, None),
    "random_self_loops": (lambda: random_graph(self_loops=True), None, None),
    "random_duplicates": (lambda: random_graph(duplicates=True), None, None),
    "hub": (hub, 260, 769),
}
