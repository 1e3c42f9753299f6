"""Plain numpy restatement of n-gram static masking for tests/test_span_static_gpu.py:
the native streams (Philox4x32-10 under part_key, CtrRng's counter layout), the partition order
of order_native_kernel, and the budgeted walk, pair by pair from the definition."""
import numpy as np

M64 = (1 << 64) - 1


def mix64(x):
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    return x ^ (x >> 31)


def part_key(native_seed, part_seed):
    return mix64(native_seed ^ mix64((part_seed + 0x9E3779B97F4A7C15) & M64))


def philox(blk, id0, id1, key):
    """Philox4x32-10 at counters (blk[i], id0, id1, 0x6C64646C): uint64 [len(blk), 4]."""
    c = [blk.astype(np.uint64), np.full(len(blk), id0, np.uint64), np.full(len(blk), id1, np.uint64),
         np.full(len(blk), 0x6C64646C, np.uint64)]
    k0, k1 = key & 0xFFFFFFFF, key >> 32
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(0xD2511F53), c[2] * np.uint64(0xCD9E8D57)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(0xFFFFFFFF),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(0xFFFFFFFF)]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, 1)


def planner_index(k, n_pairs, key):
    """Output row k of a partition of n_pairs pairs -> its planner index (order_native_kernel)."""
    key = mix64(key ^ 3)
    bits = 1
    while (1 << bits) < n_pairs:
        bits += 1
    h = (bits + 1) >> 1
    hm = (1 << h) - 1
    x = k
    while True:
        L, R = x >> h, x & hm
        for rd in range(4):
            L, R = R, L ^ (mix64(R ^ key ^ (rd << 56)) & hm)
        x = (L << h) | R
        if x < n_pairs:
            return x


def mask_pair(orig, na, budget, key, idx, cum, cls_id, sep_id, cont_vocab, stats):
    """Masked token indices (sorted) of one pair by the walk of DESIGN §27; counts the paths taken
    in `stats`. cum: the 15 float32 of lddl_span_params."""
    n = len(orig)
    special = (orig == cls_id) | (orig == sep_id)
    first = np.zeros(n, bool)
    first[[0, na]] = True
    cont = ~special & ~first & ~np.concatenate([[True], special[:-1]]) & cont_vocab[orig]
    heads = np.flatnonzero(~special & ~cont)
    W = len(heads)
    cumtok = np.concatenate([np.cumsum(~special)[heads] - 1, [int((~special).sum())]])
    ends = np.concatenate([heads, [n]])
    r = philox(heads.astype(np.uint64) << np.uint64(16), idx & 0xFFFFFFFF, (idx >> 32) << 4 | 5, key)
    u = ((r[:, 1] >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0))
    L = 1 + (u[:, None] >= cum[None, :]).sum(1)
    covered = np.zeros(W, bool)
    masked = np.zeros(n, bool)
    m = 0
    for j in sorted(range(W), key=lambda j: (int(r[j, 0]), int(heads[j]) % 64, int(heads[j]))):
        if m == budget:
            break
        if covered[j]:
            continue
        n0 = g = min(int(L[j]), W - j)
        while g >= 1 and m + cumtok[j + g] - cumtok[j] > budget:
            g -= 1
        stats['shrunk'] += 0 < g < n0
        stats['shrunk_to_0'] += g == 0
        if g == 0:
            continue
        if covered[j:j + g].any():
            stats['overlap'] += 1
            continue
        covered[j:j + g] = True
        masked[ends[j]:ends[j + g]] = True
        m += cumtok[j + g] - cumtok[j]
        stats['ab'] += ends[j] < na <= heads[j + g - 1]
        stats['slot64'] += ends[j] <= 63 and ends[j + g] > 64
        stats['special_inside'] += bool(special[ends[j]:heads[j + g - 1]].any())
    masked &= ~special
    assert masked.sum() == m
    stats['below'] += m < budget
    return np.flatnonzero(masked)


def expect(plain, orig_all, span_cum, native_seed, part_seeds, cls_id, sep_id, cont_vocab):
    """(pos, labels, pos_off, stats) of the span run over the pairs of the per-token native run
    `plain` (make_pairs(...).to_host()); orig_all: its tokens with the labels put back."""
    tok_off, len_a, po = plain['tok_off'], plain['len_a'], plain['part_off']
    budget = np.diff(plain['pos_off'])
    stats = dict.fromkeys(('shrunk', 'shrunk_to_0', 'overlap', 'ab', 'slot64', 'special_inside',
                           'below'), 0)
    pos, lab, cnt = [], [], []
    for p in range(len(po) - 1):
        key = part_key(native_seed, int(part_seeds[p]))
        for q in range(po[p], po[p + 1]):
            orig, na = orig_all[tok_off[q]:tok_off[q + 1]], int(len_a[q])
            idx = planner_index(int(q - po[p]), int(po[p + 1] - po[p]), key)
            t = mask_pair(orig, na, int(budget[q]), key, idx, span_cum, cls_id, sep_id, cont_vocab,
                          stats)
            pos.append(np.where(t < na, t + 1, t + 2))
            lab.append(orig[t])
            cnt.append(len(t))
    return (np.concatenate(pos).astype(np.uint16), np.concatenate(lab),
            np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), stats)
