"""A numpy restatement of the rules every ranking kernel of the library selects by, written from the
rules and not from the kernels:

  order key    a float32 maps to an unsigned 32-bit key with the same order: a value with the sign bit clear gets it set, a
               value with the sign bit set has all its bits inverted.  -Inf < negatives < -0.0 < +0.0 < positives < +Inf; the
               two zeros are DIFFERENT keys, -0.0 the lower one.  The inverse gives the float back bit for bit.
  schedule     the radix selection reads the keys in digits of (up to) eight bits, the most significant first.  Bits above the
               highest bit in which the smallest and the largest key differ are shared by all keys and skipped: the first digit
               is the eight bits that end at that highest differing bit (fewer when it is below bit 7), every later digit the
               eight bits below the one before, the last one ending at bit 0.
  selection    after `limit` digits the value left is the k-th largest key with its unread low bits cleared: the lower edge of
               the bin that holds the k-th largest key.  With all digits read it is that key; when all keys are equal it is
               that key as well and no digit is read.

No tests here (tests/test_selection_model_cpu.py)."""
import numpy as np

SIGN = np.uint32(0x80000000)


def order_key(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & SIGN, ~u, u | SIGN).astype(np.uint32)


def from_order_key(key):
    key = np.ascontiguousarray(key, dtype=np.uint32)
    return np.where(key & SIGN, key & ~SIGN, ~key).astype(np.uint32).view(np.float32)


def digit_schedule(diff):
    """[(shift, width), ...] of the digits read for keys whose smallest and largest differ in the bits `diff` (not 0)"""
    diff = int(diff)
    assert 0 < diff < 1 << 32
    top = diff.bit_length() - 1
    out, hi = [], top + 1                                      # hi: one past the highest bit not read yet
    while hi > 0:
        lo = max(hi - 8, 0)
        out.append((lo, hi - lo))
        hi = lo
    return out


def kth_largest_key(keys, k):
    keys = np.sort(np.asarray(keys, dtype=np.uint32))
    assert 1 <= k <= keys.size
    return keys[keys.size - k]


def select_key(keys, k, limit=99):
    """what the selection leaves for the k-th largest of `keys` after at most `limit` digits"""
    keys = np.asarray(keys, dtype=np.uint32)
    kth = int(kth_largest_key(keys, k))
    diff = int(keys.min()) ^ int(keys.max())
    if diff == 0:
        return np.uint32(kth)
    read = digit_schedule(diff)[:limit]
    unread = (1 << read[-1][0]) - 1                            # the bits below the last digit read
    return np.uint32(kth & ~unread)


def select_value(scores, k, limit=99):
    """the float the selection hands on as tau: the k-th largest score, or the lower edge of its bin"""
    return from_order_key(np.array([select_key(order_key(scores), k, limit)], np.uint32))[0]


def rank_by_key(pids, scores, key=order_key):
    """(pids, scores) ordered by `key` of the score descending, the lower pid first among equal keys"""
    pids, scores = np.asarray(pids, dtype=np.int64), np.asarray(scores, dtype=np.float32)
    k = np.asarray(key(scores)).astype(np.int64)
    order = np.lexsort((pids, -k))
    return pids[order], scores[order]


# ---- two mistakes a kernel can make, as keys (for the host sensitivity checks; never run on a device) --------------------
def wrong_key_unsigned_bits(x):
    """the float's bits taken as an unsigned integer: right among positives, negatives above them and reversed"""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def wrong_key_magnitude(x):
    """the sign dropped: order by |x|"""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & ~SIGN


def rank_merge(lists, k, before):
    """The rank merge of sorted shard results: a record's place is its index in its own list plus,
    for every other list, the number of records a binary search finds before it under `before(s2, p2, s, p)`.  -> the places
    of all records [(place, pid, score)]: a correct merge gives every record another place."""
    out = []
    for l, own in enumerate(lists):
        for i, (p, s) in enumerate(own):
            rank = i
            for l2, other in enumerate(lists):
                if l2 == l:
                    continue
                lo, hi = 0, len(other)
                while lo < hi:
                    mid = (lo + hi) // 2
                    p2, s2 = other[mid]
                    if before(s2, p2, s, p):
                        lo = mid + 1
                    else:
                        hi = mid
                rank += lo
            out.append((rank, p, s))
    return sorted(out, key=lambda r: (r[0], r[1]))


def before_by_float(s2, p2, s, p):
    return bool(s2 > s or (s2 == s and p2 < p))


def before_by_key(s2, p2, s, p):
    a2, a = int(order_key([s2])[0]), int(order_key([s])[0])
    return a2 > a or (a2 == a and p2 < p)
