"""The prefix cache's keys restated in numpy (star-vector_amd/csrc/prefix_cache/prefix_cache.hip states the rule in its header).

A full page of a prompt = 64 consecutive rows of `hidden` bf16 = 16 * hidden little-endian 64-bit words w_i.  With splitmix64's finaliser
mix64 and three constants, all arithmetic mod 2^64:
    digest.a = SUM_i mix64(w_i + (i + 1) * C1)          digest.b = XOR_i mix64((w_i ^ C3) + (i + 1) * C2)
    key_k.a  = mix64((key_{k-1}.a ^ d_k.a) + C1)        key_k.b  = mix64((key_{k-1}.b + d_k.b) ^ key_k.a)        key_{-1} = KEY0
An admit reuses h = min(leading keys found in the table, (L - 1) // 64) pages of a prompt of L rows."""
import numpy as np

PAGE = 64
M64 = (1 << 64) - 1
C1, C2, C3 = 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9
KEY0 = (0x5356505243414348, 0x7061676564696731)


def mix64_np(x):
    x = x.astype(np.uint64)
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def mix64(x):
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def page_digest(page_u16):
    """page_u16: the [64, hidden] bf16 bit patterns of one page as uint16 -> (a, b)"""
    w = np.ascontiguousarray(page_u16, dtype="<u2").reshape(-1).view("<u8").astype(np.uint64)
    with np.errstate(over="ignore"):
        i = np.arange(1, w.size + 1, dtype=np.uint64)
        a = mix64_np(w + i * np.uint64(C1))
        b = mix64_np((w ^ np.uint64(C3)) + i * np.uint64(C2))
        return int(np.add.reduce(a, dtype=np.uint64)), int(np.bitwise_xor.reduce(b))


def prompt_digests(rows_u16):
    """rows_u16 [L, hidden] uint16 -> the digests of its L // 64 full pages"""
    return [page_digest(rows_u16[PAGE * k:PAGE * (k + 1)]) for k in range(rows_u16.shape[0] // PAGE)]


def chain(prev, d):
    a = mix64(((prev[0] ^ d[0]) + C1) & M64)
    return a, mix64(((prev[1] + d[1]) & M64) ^ a)


def keys_of(digests):
    out, key = [], KEY0
    for d in digests:
        key = chain(key, d)
        out.append(key)
    return out


def hit_pages(digests, L, table):
    """pages an admit of a prompt of L rows reuses against `table`, a set of keys"""
    matched = 0
    for key in keys_of(digests):
        if key not in table:
            break
        matched += 1
    return min(matched, (L - 1) // PAGE)
