"""T5 span corruption as include/lddl_amd.h states it, written sequentially in
plain Python: sort the keys, walk the segments, append to lists. Shares no code with the product
but the Philox of denoise_oracle.py; the block's tokens come from blocks_oracle.py."""
import math

import numpy as np

import blocks_oracle as BO
from denoise_oracle import philox


def fixed(noise_density, mean_noise_span_length, n_sentinels):
    """(dq, iq, n_sentinels): the two floats in 16.16 fixed point, rounded half up."""
    return (int(math.floor(noise_density * 65536 + 0.5)),
            int(math.floor(65536 / mean_noise_span_length + 0.5)), n_sentinels)


def counts(n, dq, iq, n_sentinels):
    """(N, k): noise tokens and spans of a row of n tokens."""
    if n < 2:
        return 0, 0
    N = min(max((n * dq + 32768) >> 16, 1), n - 1)
    return N, min(max((N * iq + 32768) >> 16, 1), min(N, n - N, n_sentinels))


def lengths(n, dq, iq, n_sentinels):
    N, k = counts(n, dq, iq, n_sentinels)
    return n - N + k + 1, N + k + 1


def ranked(keys, count):
    """Items 1 .. count - 1 by (key, item); keys[u] belongs to item u + 1."""
    return sorted(range(1, count), key=lambda j: (keys[j - 1], j))


def row_keys(i, n, L, q, seed, counter):
    """(N, k, noise keys, non-noise keys) of row i; q = (dq, iq, n_sentinels)."""
    N, k = counts(n, *q)
    r = [philox(i * L + u, counter, seed) for u in range(max(N, n - N) - 1)]
    return N, k, [x[0] >> 8 for x in r], [x[1] >> 8 for x in r]


def corrupt_row(i, t, L, in_len, tgt_len, q, *, sentinel_first, eos, pad, dec_start, ignore, seed,
                counter):
    """Row i from its tokens t -> its six outputs in t5_corrupt's order, and t's noise mask."""
    n = len(t)
    N, k, kn, km = row_keys(i, n, L, q, seed, counter)
    B = [0] + sorted(ranked(kn, N)[:k - 1]) + [N]
    A = [0] + sorted(ranked(km, n - N)[:k - 1]) + [n - N]
    inp, lab, noise, pos = [] if k else list(t), [], [0] * (n if not k else 0), 0
    for g in range(k):  # the clean segment and its sentinel, the sentinel and its noise
        a, b = A[g + 1] - A[g], B[g + 1] - B[g]
        inp += t[pos:pos + a] + [sentinel_first - g]
        lab += [sentinel_first - g] + t[pos + a:pos + a + b]
        noise += [0] * a + [1] * b
        pos += a + b
    assert len(noise) == n and len(inp) == n - N + k and len(lab) == N + k
    inp, lab = inp[:in_len - 1] + [eos], lab[:tgt_len - 1] + [eos]
    att = [1] * len(inp) + [0] * (in_len - len(inp))
    dec = ([dec_start] + lab + [pad] * tgt_len)[:tgt_len]
    return (inp + [pad] * (in_len - len(inp)), att, lab + [ignore] * (tgt_len - len(lab)), dec,
            n - N + k + 1, N + k + 1, noise)


def corrupt(ids, sent_off, P, sep, blocks, rows, L, in_len, tgt_len, q, **kw):
    """The batch as t5_corrupt's dict of numpy arrays, and per row (tokens, noise mask)."""
    toks = [[t for t, _, _ in BO.block_slots(ids, sent_off, P, sep, blocks[k], 0, 0, kw['eos'],
                                             0)[0][1:-1]]
            for k in (range(len(blocks)) if rows is None else rows)]
    res = [corrupt_row(i, t, L, in_len, tgt_len, q, **kw) for i, t in enumerate(toks)]
    out = {k: np.array([r[j] for r in res], np.int64) for j, k in enumerate(
        'input_ids attention_mask labels decoder_input_ids src_lengths tgt_lengths'.split())}
    return out, [(t, r[6]) for t, r in zip(toks, res)]
