"""BART denoising as include/lddl_amd.h states it, written sequentially in plain
Python and numpy: sort the units, walk the words, append to a list. Shares no code with the
product; its Philox4x32-10 takes the collates' counter layout."""
import numpy as np

M32 = 0xFFFFFFFF
SPAN_XOR, SENT_XOR = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
LEN_MASK, S_MAX = (1 << 30) - 1, 256


def philox(flat, counter, key):
    c = [flat & M32, (flat >> 32) & M32, counter & M32, (counter >> 32) & M32]
    k0, k1 = key & M32, (key >> 32) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def u01(v):  # exact in double, as in float32
    return (v >> 8) / 16777216.0


def denoise_row(i, sents, L, cont, *, bos, eos, pad, mask_id, dec_start, ignore, vocab_len, seed,
                counter, stride, permute_p, random_ratio, p_start, cum):
    """Row i of a batch from the sample's sentences (lists of ids) -> (input_ids, attention_mask,
    decoder_input_ids, labels, src_length, events). cum: the 16 float32 entries as floats."""
    left, kept = L - 2, []
    for s in sents:  # the budget: the first L - 2 pieces in original order
        kept.append(list(s[:left]))
        left -= len(kept[-1])
    units = [[s] for s in kept[:S_MAX - 1]] + ([kept[S_MAX - 1:]] if len(kept) >= S_MAX else [])
    rs = [philox(i * stride + u, counter, seed ^ SENT_XOR) for u in range(len(units))]
    part = [u for u in range(len(units))
            if sum(map(len, units[u])) and u01(rs[u][0]) < permute_p]
    placed = list(range(len(units)))
    for place, u in zip(part, sorted(part, key=lambda u: (rs[u][1], u))):
        placed[place] = u
    seq = [(t, k == 0) for u in placed for s in units[u] for k, t in enumerate(s)]
    out, events = [], set()
    c = 0               # words from here on that a span started before still reaches
    keep_rest = True    # whether the current word's continuations keep their ids
    prev_noised = False  # the word before was deleted or replaced
    for x, (t, first) in enumerate(seq):
        if not (first or not cont[t]):
            if keep_rest:
                out.append(t)
            if x % 64 == 0:
                events.add('word straddles two windows')
            if not keep_rest and x == 64:
                events.add('span across slots 63 / 64')
            continue
        r = philox(i * stride + x, counter, seed)
        ln = -1
        if u01(r[0]) < p_start:
            v = u01(philox(i * stride + x, counter, seed ^ SPAN_XOR)[0])
            ln = sum(v >= ck for ck in cum)
        noise = (r[3] * vocab_len) >> 32 if u01(r[1]) < random_ratio else mask_id
        if c > 0:  # deleted: the run already has its noise token
            if first:
                events.add('span crosses a sentence boundary')
            if x == 64:
                events.add('span across slots 63 / 64')
        elif ln >= 1:
            out.append(noise)
            if prev_noised:
                events.add('two adjacent spans, two masks')
        elif ln == 0:
            out += [noise, t]
        else:
            out.append(t)
        keep_rest = c == 0 and ln < 1
        prev_noised = c > 0 or ln >= 1
        c = max(c - 1, ln - 1, 0)
    orig = [t for s in kept for t in s]
    row = [bos] + out[:L - 2] + [eos]
    att = [1] * len(row) + [0] * (L - len(row))
    row += [pad] * (L - len(row))
    labels = [bos] + orig + [eos]
    labels += [ignore] * (L - len(labels))
    dec = [dec_start] + [pad if v == ignore else v for v in labels[:-1]]
    return row, att, dec, labels, len(out) + 2, events


def denoise(ids, sent_off, sent_len, doc_sent_off, rows, L, cont, **kw):
    """The batch: dict of numpy arrays like bart_denoise's, and per row the events."""
    rows = range(len(doc_sent_off) - 1) if rows is None else rows
    res = []
    for i, d in enumerate(rows):
        sents = [[int(v) for v in ids[sent_off[s]:sent_off[s] + (int(sent_len[s]) & LEN_MASK)]]
                 for s in range(doc_sent_off[d], doc_sent_off[d + 1])]
        res.append(denoise_row(i, sents, L, cont, **kw))
    out = {k: np.array([r[j] for r in res], np.int64).reshape(len(res), L)
           for j, k in enumerate(('input_ids', 'attention_mask', 'decoder_input_ids', 'labels'))}
    out['src_lengths'] = np.array([r[4] for r in res], np.int32)
    return out, [r[5] for r in res]


def solve_p_start(ratio, weights, iters=200):
    """Bisection in double of 1 - prod_k (1 - s * P(len > k)) = ratio, weights for 0 .. n."""
    q = 1.0 - np.cumsum(np.asarray(weights, np.float64) / np.sum(weights))[:-1]
    lo, hi = 0.0, 1.0
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if 1.0 - np.prod(1.0 - mid * q) < ratio else (lo, mid)
    return 0.5 * (lo + hi)
