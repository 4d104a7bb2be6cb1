"""rl_amd.digest_model, the numpy restatement of rl_limiter_digest's definition (include/rl_engine.h):
literal known answers worked out with Python integers, and the algebra the GPU tests rely on."""
import numpy as np
import pytest

import rl_amd

M = (1 << 64) - 1
T = 1_700_000_000_000
KA, KB = 0x0123456789ABCDEF, 0xFEDCBA9876543210


def mix(x):
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M
    return x ^ (x >> 31)


def rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M


def entry_hash(key_hash, kind, f1, f2, f3):
    """The header's formula in Python integers; kind 0 SW bucket, 1 TB bucket, 2 cache entry."""
    k = (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9)[kind]
    u = (mix(key_hash) + k) & M
    u = ((u ^ (f1 & M)) * 0xFF51AFD7ED558CCD) & M
    u = ((u ^ rotl(f2 & M, 23)) * 0xC4CEB9FE1A85EC53) & M
    u ^= rotl(f3 & M, 47)
    return mix(u)


def sw(key, w0, count, exp, lim=0):
    return (lim, key, 0, w0, count, 0.0, 0, exp)


def tb(key, tokens, last, exp, lim=1):
    return (lim, key, 1, 0, 0, tokens, last, exp)


def one(entries, cache=(), shards=1):
    d = rl_amd.digest_model(entries, cache, shards, 0)
    assert d.shape == (1,)
    return int(d["entries"][0]), int(d["sum"][0]), int(d["xr"][0])


def test_known_answer_a_sliding_window_key_with_two_buckets():
    a, b = 0x1641D5E92DB5DADA, 0x50D00BCDC99CA5A7
    assert entry_hash(KA, 0, T, 3, T + 1400) == a
    assert entry_hash(KA, 0, T + 1000, 2, T + 2350) == b
    got = one([sw(KA, T, 3, T + 1400), sw(KA, T + 1000, 2, T + 2350)])
    assert got == (2, 0x6711E1B6F7528081, 0x4691DE24E4297F7D) == (2, (a + b) & M, a ^ b)


def test_known_answer_a_token_bucket_with_a_negative_zero_balance():
    h = 0x3E13888EBD945C8E
    assert entry_hash(KB, 1, 0x8000000000000000, T + 123, T + 2123) == h
    assert one([tb(KB, -0.0, T + 123, T + 2123)]) == (1, h, h)
    # the balance is hashed by its bits: +0.0 is another state
    h0 = 0x2FCF8312B62C8576
    assert entry_hash(KB, 1, 0, T + 123, T + 2123) == h0
    assert one([tb(KB, 0.0, T + 123, T + 2123)]) == (1, h0, h0)


def test_known_answer_key_hash_zero_with_a_cache_entry():
    c, s = 0xFA3D5E6273C94D32, 0xE9E1A239DCD46D22
    assert mix(0) == 0                                        # the tag of key 0 is 0
    assert entry_hash(0, 2, T + 400, 0, 0) == c
    assert entry_hash(0, 0, T, 1, T + 1010) == s
    assert one([], [(0, T + 400)]) == (1, c, c)
    assert one([sw(0, T, 1, T + 1010)], [(0, T + 400)]) == (2, 0xE41F009C509DBA54, 0x13DCFC5BAF1D2010)
    assert one([sw(0, T, 1, T + 1010)], [(0, T + 400)]) == (2, (c + s) & M, c ^ s)


def population(seed=3, n=400):
    rng = np.random.default_rng(seed)
    keys = [0, M] + [int(x) for x in rng.integers(0, 1 << 64, n - 2, dtype=np.uint64)]
    ent, cache = [], []
    for i, k in enumerate(keys):
        if i % 3 == 0:
            ent.append(tb(k, float(rng.random() * 10), T + int(rng.integers(0, 999)), T + 2000 + i))
        else:
            ent.append(sw(k, T, int(rng.integers(1, 9)), T + 1000 + i))
            if i % 2:
                ent.append(sw(k, T + 1000, int(rng.integers(1, 9)), T + 2000 + i))
        if i % 7 == 0:
            cache.append((k, T + 300 + i))
    return ent, cache


def by_int(ent, cache, shards, bits):
    """The whole model in Python integers."""
    s = shards.bit_length() - 1
    out = [[0, 0, 0] for _ in range(1 << bits)]
    items = [(e[1], e[2], (int(np.array([e[5]], "<f8").view("<u8")[0]), e[6], e[7]) if e[2]
              else (e[3], e[4], e[7])) for e in ent]
    items += [(k, 2, (x, 0, 0)) for k, x in cache]
    for k, kind, f in items:
        b = ((mix(k) << s) & M) >> (64 - bits) if bits else 0
        h = entry_hash(k, kind, *f)
        out[b][0] += 1
        out[b][1] = (out[b][1] + h) & M
        out[b][2] ^= h
    return [tuple(x) for x in out]


def as_tuples(d):
    return [(int(a), int(b), int(c)) for a, b, c in zip(d["entries"], d["sum"], d["xr"])]


@pytest.mark.parametrize("shards", [1, 2, 8])
def test_the_bucket_is_the_bits_below_the_shard_bits(shards):
    ent, cache = population()
    for bits in (0, 1, 3, 6):
        got = as_tuples(rl_amd.digest_model(ent, cache, shards, bits))
        assert got == by_int(ent, cache, shards, bits), (shards, bits)
    # one key: exactly the bucket spelled out in bits
    tag = mix(KA)
    s = shards.bit_length() - 1
    want = int(format(tag, "064b")[s:s + 3], 2)
    d = rl_amd.digest_model([sw(KA, T, 3, T + 1400)], [], shards, 3)
    assert [i for i in range(8) if d["entries"][i]] == [want]
    # a coarser digest is the finer one folded pairwise (buckets are prefixes)
    fine = rl_amd.digest_model(ent, cache, shards, 4)
    coarse = rl_amd.digest_model(ent, cache, shards, 3)
    np.testing.assert_array_equal(coarse["entries"], fine["entries"][0::2] + fine["entries"][1::2])
    np.testing.assert_array_equal(coarse["xr"], fine["xr"][0::2] ^ fine["xr"][1::2])
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal(coarse["sum"], fine["sum"][0::2] + fine["sum"][1::2])


def test_the_model_does_not_depend_on_the_order():
    ent, cache = population()
    want = rl_amd.digest_model(ent, cache, 1, 3).tobytes()
    rng = np.random.default_rng(8)
    for _ in range(3):
        e2 = [ent[i] for i in rng.permutation(len(ent))]
        c2 = [cache[i] for i in rng.permutation(len(cache))]
        assert rl_amd.digest_model(e2, c2, 1, 3).tobytes() == want


def test_the_model_is_additive_over_a_split_of_the_entries():
    ent, cache = population()
    whole = rl_amd.digest_model(ent, cache, 2, 3)
    cut, ccut = len(ent) // 3, len(cache) // 2
    a = rl_amd.digest_model(ent[:cut], cache[ccut:], 2, 3)
    b = rl_amd.digest_model(ent[cut:], cache[:ccut], 2, 3)
    np.testing.assert_array_equal(whole["entries"], a["entries"] + b["entries"])
    np.testing.assert_array_equal(whole["xr"], a["xr"] ^ b["xr"])
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal(whole["sum"], a["sum"] + b["sum"])
    empty = rl_amd.digest_model([], [], 1, 3)
    assert empty.shape == (8,) and not empty.view(np.uint64).any()


def test_one_changed_field_changes_exactly_that_buckets_sum_and_xr():
    ent, cache = population()
    base = rl_amd.digest_model(ent, cache, 1, 3)

    def differs_only_in(d, key):
        b = mix(key) >> 61
        others = [i for i in range(8) if i != b]
        assert d[others].tobytes() == base[others].tobytes()
        assert d["entries"][b] == base["entries"][b]
        assert d["sum"][b] != base["sum"][b] and d["xr"][b] != base["xr"][b]

    i_sw = next(i for i, e in enumerate(ent) if e[2] == 0)
    i_tb = next(i for i, e in enumerate(ent) if e[2] == 1)
    for i, field, new in ((i_sw, 3, T + 2000), (i_sw, 4, ent[i_sw][4] + 1), (i_sw, 7, ent[i_sw][7] + 1),
                          (i_tb, 5, ent[i_tb][5] + 0.5), (i_tb, 6, ent[i_tb][6] + 1),
                          (i_tb, 7, ent[i_tb][7] + 1)):
        e2 = list(ent)
        e2[i] = ent[i][:field] + (new,) + ent[i][field + 1:]
        differs_only_in(rl_amd.digest_model(e2, cache, 1, 3), ent[i][1])
    c2 = list(cache)
    c2[1] = (cache[1][0], cache[1][1] + 1)
    differs_only_in(rl_amd.digest_model(ent, c2, 1, 3), cache[1][0])
    # the same fields under another kind, and swapped fields, are other entries
    assert entry_hash(KA, 0, 5, 0, 0) != entry_hash(KA, 2, 5, 0, 0) != entry_hash(KA, 1, 5, 0, 0)
    assert entry_hash(KA, 0, 5, 9, 0) != entry_hash(KA, 0, 9, 5, 0)
    assert one([sw(KA, 5, 9, 7)]) != one([sw(KA, 9, 5, 7)]) != one([sw(KA, 5, 7, 9)])
