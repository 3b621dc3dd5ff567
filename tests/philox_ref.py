"""The production noise contract in numpy: which Philox4x32-10 counter every device draw reads, and how its words become a
uniform or a normal.  Written from the documented contract (dd_step.hip's header comment, include/decompdiff_hip_debug.h,
the sample_diffusion docstring) and the published definition of Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy
as 1, 2, 3", SC'11; the Random123 known answers are checked in tests/test_philox_ref_host.py) -- not from the kernel source.  A
plain helper module (no tests): tests/test_philox_ref_host.py checks it on the host, tests/test_gpu_philox_contract.py and
tests/philox_step_cases.py hold the device to it.

    key      (seed & 0xffffffff, seed >> 32)
    counter  types:        (row & 0xffffffff, row >> 32, time word, stream | block << 8); class c is word c % 4 of block c // 4
             coordinates:  (idx, 0, time word, stream), idx = 3 * atom + axis flat over the batch
    time     t + 65536 * epoch as a uint32 (epoch 0: t itself; a chain init: the level drawn)
    streams  step 1 atom types / 2 bond types / 7 coordinates, jump 3 / 4 / 8, chain init 5 / 6 / 9
    uniform  (word >> 8) * 2^-24
    normal   sqrt(-2 log max(u1, 2^-24)) cos(fl32(2 pi) *_fp32 u2) from words 0 and 1 of the block
A keyed chain uses the sample's key as the seed and the rows of the sample's own enumeration: the same functions."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57                 # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85                 # key increments (Weyl constants)
MASK = 0xFFFFFFFF
STEP_STREAMS, JUMP_STREAMS, INIT_STREAMS = (1, 2, 7), (3, 4, 8), (5, 6, 9)      # (atom types, bond types, coordinates)
NUM_BOND_CLASSES = 5
U_MIN = 2.0 ** -24                              # the clamp of u1, and the spacing of the uniforms
TWO_PI_F32 = np.float32(6.283185307179586)


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds of Philox4x32 on arrays of 32-bit words held in uint64 -> four uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(x) & _u64(MASK) for x in (c0, c1, c2, c3, k0, k1)))
    m32, sh = np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & m32, (p0 >> sh) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(W0)) & m32, (k1 + np.uint64(W1)) & m32
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def key_of(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & MASK, seed >> 32


def time_word(t, epoch=0):
    return (int(t) + 65536 * int(epoch)) & MASK


def class_counter(row, word, stream, c):
    """Counter words of class c of a type row."""
    return int(row) & MASK, int(row) >> 32, int(word) & MASK, int(stream) | ((int(c) // 4) << 8)


def coord_counter(idx, word, stream):
    return int(idx) & MASK, 0, int(word) & MASK, int(stream)


def uniform_words(seed, rows, word, stream, nc):
    """uint32 [rows, nc]: the word behind every class of rows 0..rows-1 (`rows` may also be an array of row numbers)."""
    k0, k1 = key_of(seed)
    r = np.arange(rows, dtype=np.uint64) if np.isscalar(rows) else _u64(rows)
    out = np.empty((r.size, nc), dtype=np.uint32)
    for blk in range((nc + 3) // 4):
        w = philox4x32_10(r & np.uint64(MASK), r >> np.uint64(32), int(word) & MASK, int(stream) | (blk << 8), k0, k1)
        for k in range(min(4, nc - 4 * blk)):
            out[:, 4 * blk + k] = w[k]
    return out


def uniforms(seed, rows, word, stream, nc):
    """float32 [rows, nc] in [0, 1 - 2^-24]; (w >> 8) * 2^-24 is exact in fp32."""
    return ((uniform_words(seed, rows, word, stream, nc) >> np.uint32(8)).astype(np.float64) * U_MIN).astype(np.float32)


def normal_words(seed, n, word, stream):
    """(word 0, word 1) of the blocks of coordinates 0..n-1 (or of an array of indices)."""
    k0, k1 = key_of(seed)
    idx = np.arange(n, dtype=np.uint64) if np.isscalar(n) else _u64(n)
    w = philox4x32_10(idx, 0, int(word) & MASK, int(stream), k0, k1)
    return w[0], w[1]


def normals(seed, n, word, stream):
    """Box-Muller normals of coordinates 0..n-1 -> dict(z64, z64a, z32, u1, u2): pure float64; float64 with the angle taken as the
    fp32 product fl32(2 pi) * u2 (that rounding belongs to the draw's definition); every operation in numpy float32."""
    w0, w1 = normal_words(seed, n, word, stream)
    u1 = np.maximum((w0 >> np.uint32(8)).astype(np.float64) * U_MIN, U_MIN)
    u2 = (w1 >> np.uint32(8)).astype(np.float64) * U_MIN
    r64 = np.sqrt(-2.0 * np.log(u1))
    z64 = r64 * np.cos(2.0 * np.pi * u2)
    ang32 = TWO_PI_F32 * u2.astype(np.float32)                           # fp32 x fp32 -> fp32, one rounding
    assert ang32.dtype == np.float32
    z64a = r64 * np.cos(ang32.astype(np.float64))
    u1f = u1.astype(np.float32)
    z32 = np.sqrt(np.float32(-2.0) * np.log(u1f)) * np.cos(ang32)
    assert z32.dtype == np.float32
    return dict(z64=z64, z64a=z64a, z32=z32, u1=u1, u2=u2)


def step_draws(seed, t, n_lig, n_bond, nc):
    """The noise of the plain reverse step at time t (epoch 0) in the layout injected ``noise=`` takes, as numpy float32:
    u_v [n_lig, nc] (stream 1), u_b [n_bond, 5] (stream 2), eps [n_lig, 3] (stream 7, z32)."""
    word = time_word(t)
    return dict(u_v=uniforms(seed, n_lig, word, STEP_STREAMS[0], nc), u_b=uniforms(seed, n_bond, word, STEP_STREAMS[1], NUM_BOND_CLASSES),
                eps=normals(seed, 3 * n_lig, word, STEP_STREAMS[2])["z32"].reshape(n_lig, 3))


def chain_counters(B, NL, nc, T, epochs):
    """Every counter (as one Python int of 128 bits: c0 | c1 << 32 | c2 << 64 | c3 << 96, in a uint64 pair array [n, 2]) that one
    resampled chain with init= may read under one key: steps (streams 1 / 2 / 7) at t = 0..T-1 in every epoch, jumps (3 / 4 / 8)
    to a level 0..T-1 in every epoch, the chain init (5 / 6 / 9) at level 0..T (T: the prior).  From the addressing above alone."""
    n_atom, n_bond, n_xyz = B * NL, B * NL * (NL - 1), 3 * B * NL
    parts = []

    def add(rows, words, stream, nblk):
        r = np.arange(rows, dtype=np.uint64)
        w = _u64(words)
        for blk in range(nblk):
            c3 = np.uint64(stream | (blk << 8))
            lo = (r[None, :] | np.zeros((w.size, 1), np.uint64)).ravel()            # c0 | c1 << 32 = the row itself
            hi = (w[:, None] | (c3 << np.uint64(32)) | np.zeros((1, rows), np.uint64)).ravel()
            parts.append(np.stack([lo, hi], 1))

    step_words = [time_word(t, e) for e in range(epochs) for t in range(T)]
    jump_words = [time_word(t, e) for e in range(1, epochs + 1) for t in range(T)]     # (the epoch AFTER the jump)
    init_words = [time_word(t) for t in range(T + 1)]
    nbv, nbb = (nc + 3) // 4, (NUM_BOND_CLASSES + 3) // 4
    for streams, words in ((STEP_STREAMS, step_words), (JUMP_STREAMS, jump_words), (INIT_STREAMS, init_words)):
        add(n_atom, words, streams[0], nbv)
        add(n_bond, words, streams[1], nbb)
        add(n_xyz, words, streams[2], 1)
    return np.concatenate(parts, 0)


# ---------------------------------------------------------------- the draws tests/test_gpu_philox_contract.py asks the device for
CONTRACT_SEEDS = (0, 2021, 1 << 32, 0x9E3779B97F4A7C15, 2 ** 64 - 1)
CONTRACT_WORDS = (0, 999, 65535, 5 + 65536 * 3, 0x7FFFFFFF, 0x80000005)    # (the last reaches the C ABI as a negative int)
CONTRACT_CLASS_COUNTS = (0, 8, 13, 23)                                      # of kinds 1 / 3 / 5; 0 means 8
ATOM_KINDS, BOND_KINDS, NORMAL_KINDS = (1, 3, 5), (2, 4, 6), (7, 8, 9)
ATOM_ROWS, BOND_ROWS, N_NORMALS = 300, 1000, 1000
# (seed, stream, position) at time word 500 whose draw sits on an edge: u1 bits all zero (the clamp is taken) / u exactly 0 /
# u = 1 - 2^-24.  Found by a host search over 2^22 counters each; tests/test_philox_ref_host.py re-derives every one.
EDGE_WORD = 500
EDGE_NORMALS = ((44713, 7, 56), (102034, 8, 55), (186393, 9, 25))           # idx
EDGE_UNIFORMS = ((44275, 1, 34, 3, 0.0), (84380, 1, 61, 1, 1.0 - U_MIN))    # row, class, value


def as_c_int(word):
    """A time word as the C int dd_debug_philox takes."""
    word = int(word) & MASK
    return word - (1 << 32) if word >= 1 << 31 else word


_D32A = []


def contract_d32a():
    """max |z32 - z64a| over every normal the GPU test compares (kinds 7-9 x CONTRACT_SEEDS x CONTRACT_WORDS x N_NORMALS draws and
    the three edge draws): what fp32 arithmetic alone costs the reference on those draws."""
    if not _D32A:
        d = 0.0
        for stream in NORMAL_KINDS:
            for seed in CONTRACT_SEEDS:
                for word in CONTRACT_WORDS:
                    n = normals(seed, N_NORMALS, word, stream)
                    d = max(d, float(np.abs(n["z32"].astype(np.float64) - n["z64a"]).max()))
        for seed, stream, idx in EDGE_NORMALS:
            n = normals(seed, np.array([idx]), EDGE_WORD, stream)
            d = max(d, float(np.abs(n["z32"].astype(np.float64) - n["z64a"]).max()))
        _D32A.append(d)
    return _D32A[0]
