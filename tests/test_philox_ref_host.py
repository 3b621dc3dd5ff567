"""Host checks of tests/philox_ref.py, the numpy restatement of the production noise contract: the published known answers of
Philox4x32-10, the uniform and Box-Muller conversions, the key-half order, that no two draws of a chain share a counter, the
edge draws the GPU test asks the device for (re-derived here), and d32a -- what fp32 arithmetic alone costs the reference's
normals, the unit of the GPU test's bound.  No GPU, no library."""
import numpy as np
import pytest

import philox_ref as PR

# Random123's known answers for philox4x32-10: counter words, key words, output words
KAT = (
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
)


def _hex(s):
    return [int(x, 16) for x in s.split()]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_philox4x32_10_known_answers(ctr, key, out):
    got = PR.philox4x32_10(*_hex(ctr), *_hex(key))
    assert all(g.dtype == np.uint32 for g in got)
    assert [int(g) for g in got] == _hex(out)


def test_known_answers_vectorised():
    """The same three as ONE call on arrays: the broadcasting of the reference is part of what every later test relies on."""
    c = np.array([_hex(k[0]) for k in KAT], dtype=np.uint64)
    k = np.array([_hex(k[1]) for k in KAT], dtype=np.uint64)
    got = np.stack(PR.philox4x32_10(c[:, 0], c[:, 1], c[:, 2], c[:, 3], k[:, 0], k[:, 1]), 1)
    assert np.array_equal(got, np.array([_hex(k[2]) for k in KAT], dtype=np.uint32))


def test_uniforms_are_the_top_24_bits():
    for nc in (5, 8, 13, 23):
        w = PR.uniform_words(2021, 4096, 999, 1, nc)
        u = PR.uniforms(2021, 4096, 999, 1, nc)
        assert u.dtype == np.float32 and u.shape == (4096, nc)
        assert float(u.min()) >= 0.0 and float(u.max()) <= 1.0 - 2.0 ** -24
        assert np.array_equal((u.astype(np.float64) * 2.0 ** 24).astype(np.uint32), w >> np.uint32(8))     # exact in fp32
    # class c is word c % 4 of block c // 4: a 13-class row is the first 13 words of its four blocks, in order
    k0, k1 = PR.key_of(2021)
    blocks = [PR.philox4x32_10(np.arange(7), 0, 999, 3 | (b << 8), k0, k1) for b in range(4)]
    flat = np.stack([w for blk in blocks for w in blk], 1)
    assert np.array_equal(PR.uniform_words(2021, 7, 999, 3, 13), flat[:, :13])
    assert np.array_equal(PR.uniform_words(2021, 7, 999, 3, 8), flat[:, :8])
    # ... and rows given as numbers address the same counters as rows 0..n-1
    assert np.array_equal(PR.uniform_words(2021, np.array([5, 2]), 999, 3, 13), flat[[5, 2], :13])


def test_key_halves_and_counter_words():
    """Key = (low half, high half) of the seed; counter = (row low, row high, time word, stream | block << 8)."""
    seed = 0x0123456789ABCDEF
    assert PR.key_of(seed) == (0x89ABCDEF, 0x01234567) and PR.key_of(-1) == (0xFFFFFFFF, 0xFFFFFFFF)
    want = PR.philox4x32_10(7, 0, 999, 1 | (2 << 8), 0x89ABCDEF, 0x01234567)
    assert [int(w) for w in want[:2]] == [int(x) for x in PR.uniform_words(seed, np.array([7]), 999, 1, 13)[0, 8:10]]
    swapped = PR.philox4x32_10(7, 0, 999, 1 | (2 << 8), 0x01234567, 0x89ABCDEF)
    assert int(swapped[0]) != int(want[0])
    assert PR.class_counter(7, 999, 1, 9) == (7, 0, 999, 1 | (2 << 8))
    assert PR.class_counter((3 << 32) | 7, 5, 2, 4) == (7, 3, 5, 2 | (1 << 8))          # rows beyond 2^32: counter word 1
    row = np.array([(3 << 32) | 7], dtype=np.uint64)
    assert int(PR.uniform_words(seed, row, 5, 2, 5)[0, 4]) == int(PR.philox4x32_10(7, 3, 5, 2 | (1 << 8), *PR.key_of(seed))[0])
    assert PR.coord_counter(56, 500, 7) == (56, 0, 500, 7)
    # the time word: t + 65536 * epoch as a uint32; the C int of a word with the top bit set is negative
    assert PR.time_word(5, 3) == 5 + 65536 * 3 and PR.time_word(999) == 999 and PR.time_word(-1) == 0xFFFFFFFF
    assert PR.as_c_int(0x80000005) == -(2 ** 31) + 5 and PR.as_c_int(0x7FFFFFFF) == 2 ** 31 - 1
    assert PR.time_word(PR.as_c_int(0x80000005)) == 0x80000005


def test_normals_three_forms():
    n = PR.normals(2021, 100000, 999, 7)
    assert n["z64"].dtype == np.float64 and n["z64a"].dtype == np.float64 and n["z32"].dtype == np.float32
    assert np.isfinite(n["z32"]).all() and float(n["u1"].min()) >= 2.0 ** -24
    assert abs(float(n["z64"].mean())) < 0.02 and abs(float(n["z64"].var()) - 1.0) < 0.02
    # the fp32 angle is one rounding of the draw's definition: it moves a draw by more than the rest of fp32 arithmetic does
    d_angle = float(np.abs(n["z64a"] - n["z64"]).max())
    d32a = float(np.abs(n["z32"] - n["z64a"]).max())
    assert 2e-7 < d32a < 1e-6 and d32a < d_angle < 3e-6, (d32a, d_angle)
    # step_draws: the injected-noise layout on streams 1 / 2 / 7
    d = PR.step_draws(2021, 999, 60, 1740, 13)
    assert d["u_v"].shape == (60, 13) and d["u_b"].shape == (1740, 5) and d["eps"].shape == (60, 3)
    assert all(v.dtype == np.float32 for v in d.values())
    assert np.array_equal(d["eps"].ravel(), n["z32"][:180]) and np.array_equal(d["u_b"], PR.uniforms(2021, 1740, 999, 2, 5))
    assert np.array_equal(d["u_v"], PR.uniforms(2021, 60, 999, 1, 13))


def test_no_two_draws_of_a_resampled_chain_share_a_counter():
    """B = 2, NL = 8, 13 classes, T = 1000, three epochs, init=: streams 1-9 over all rows, class blocks, times and epochs."""
    c = PR.chain_counters(2, 8, 13, 1000, 3)
    n_words = 3 * 1000
    want = 2 * n_words * (16 * 4 + 112 * 2 + 48) + 1001 * (16 * 4 + 112 * 2 + 48)
    assert c.shape == (want, 2)
    v = np.ascontiguousarray(c).view([("lo", np.uint64), ("hi", np.uint64)]).ravel()
    assert np.unique(v).size == want
    # the epoch never reaches into the time: T <= 65535 keeps t below the epoch's bit, and the block never reaches the stream byte
    assert PR.time_word(65535, 0) != PR.time_word(0, 1) and max(PR.STEP_STREAMS + PR.JUMP_STREAMS + PR.INIT_STREAMS) < 256


def test_edge_draws_rederived():
    """The draws the GPU test uses for the clamp of u1 and for the two ends of the uniform range are what this file says they are."""
    for seed, stream, idx in PR.EDGE_NORMALS:
        assert seed >> 32 == 0
        w0, w1 = PR.normal_words(seed, np.array([idx]), PR.EDGE_WORD, stream)
        assert int(w0[0]) >> 8 == 0, (seed, stream, idx)                      # u1 bits all zero: the clamp is taken
        n = PR.normals(seed, np.array([idx]), PR.EDGE_WORD, stream)
        assert float(n["u1"][0]) == 2.0 ** -24 and np.isfinite(n["z32"]).all()
        r = np.sqrt(-2.0 * np.log(2.0 ** -24))                                # 5.768: the largest radius a draw can have
        assert abs(float(n["z64"][0]) - r * np.cos(2.0 * np.pi * (int(w1[0]) >> 8) * 2.0 ** -24)) < 1e-12
    seed, stream, idx = PR.EDGE_NORMALS[0]
    assert int(PR.normal_words(seed, np.array([idx]), PR.EDGE_WORD, stream)[1][0]) >> 8 == 10605385
    for seed, stream, row, c, value in PR.EDGE_UNIFORMS:
        u = PR.uniforms(seed, np.array([row]), PR.EDGE_WORD, stream, 8)
        assert float(u[0, c]) == value, (seed, row, c)
    assert PR.EDGE_UNIFORMS[0][4] == 0.0 and np.float32(PR.EDGE_UNIFORMS[1][4]) == np.float32(1.0) - np.float32(2.0 ** -24)


def test_d32a_of_the_contract_draws():
    """The unit of the GPU test's bound on normals, from the reference alone: fp32 arithmetic costs the reference's own draws a
    few 1e-7 (4.7e-7 when this was written); the bound 4 x d32a then lies below 3e-6."""
    d = PR.contract_d32a()
    print(f"\nd32a over the contract draws: {d:.3g}")
    assert 1e-7 < d < 7.5e-7, d
