"""RoBERTa blocks as include/lddl_amd.h states them, written sequentially in plain
Python: walk the sentences, append to lists. Shares no code with the product but the Philox of
denoise_oracle.py, which takes the collates' counter layout."""
import numpy as np

from denoise_oracle import LEN_MASK, SPAN_XOR, philox, u01

P80 = float(np.float32(0.8))


def plan(sent_len, doc_sent_off, seq_len, mode):
    """-> (P, sep, blocks): P[n + 1], sep[n] and the emitted blocks as (first sentence, end of
    the jump, length in pieces)."""
    T, n = seq_len - 2, len(sent_len)
    ln = [int(v) & LEN_MASK for v in sent_len]
    sep, doc_end = [0] * n, [n] * n
    for d in range(len(doc_sent_off) - 1):
        a, e = int(doc_sent_off[d]), int(doc_sent_off[d + 1])
        for s in range(a, e):
            doc_end[s] = e
        full = [s for s in range(a, e) if ln[s]]
        if mode == 'full' and full:
            sep[full[-1]] = 1
    P = [0]
    for s in range(n):
        P.append(P[-1] + min(ln[s] + sep[s], T))
    blocks, b = [], 0
    while b < n:
        j, lim = b + 1, doc_end[b] if mode == 'doc' else n
        while j < lim and P[j + 1] - P[b] <= T:
            j += 1
        if P[j] > P[b]:
            blocks.append((b, j, P[j] - P[b]))
        b = j
    return P, sep, blocks


def block_slots(ids, sent_off, P, sep, block, L, bos, eos, pad):
    """The row of a block before masking: L triples (id, special, first piece of a sentence)."""
    slots = [(bos, True, False)]
    for s in range(block[0], block[1]):
        kept = P[s + 1] - P[s] - sep[s]
        slots += [(int(ids[sent_off[s] + o]), False, o == 0) for o in range(kept)]
        if sep[s]:
            slots.append((eos, True, False))
    slots.append((eos, True, False))
    real = len(slots)
    return slots + [(pad, True, False)] * (L - real), real


def collate(ids, sent_off, P, sep, blocks, rows, L, *, bos, eos, pad, mask_id=None, ignore=-100,
            vocab_len=None, mask=None, cont=None, p_start=None, cum=None):
    """The batch as collate_blocks' dict of lists, and the events of the word mode. mask = (p,
    seed, counter) with p as float32; cont and p_start / cum (15 entries) select the word mode."""
    out = {k: [] for k in ('input_ids', 'attention_mask', 'labels' if mask else 'special_tokens_mask')}
    events = set()
    for i, k in enumerate(range(len(blocks)) if rows is None else rows):
        slots, real = block_slots(ids, sent_off, P, sep, blocks[k], L, bos, eos, pad)
        out['attention_mask'].append([1] * real + [0] * (L - real))
        if not mask:
            out['input_ids'].append([t for t, _, _ in slots])
            out['special_tokens_mask'].append([int(sp) for _, sp, _ in slots])
            continue
        p, seed, counter = mask
        row, lab = [], []
        word, reach, over_sep = -1, 0, False
        for x, (t, special, first) in enumerate(slots):
            r = philox(i * L + x, counter, seed)
            masked = not special and u01(r[0]) < p
            if cum is not None:
                head = not special and (first or not cont[t])
                if head:
                    word += 1
                    if u01(r[0]) < p_start:
                        v = u01(philox(i * L + x, counter, seed ^ SPAN_XOR)[0])
                        reach = max(reach, word + 1 + sum(v >= c for c in cum))
                    if over_sep:
                        events.add('span across a separator')
                    over_sep = False
                masked = not special and reach > word
                if special and x < real - 1 and 0 <= word and reach > word + 1:
                    over_sep = True  # a span over the word before the separator reaches on
                if masked and not head and x == 64:
                    events.add('word across slots 63 / 64')
            replaced = masked and u01(r[1]) < P80
            rnd = masked and not replaced and u01(r[2]) < 0.5
            row.append(mask_id if replaced else (r[3] * vocab_len) >> 32 if rnd else t)
            lab.append(t if masked else ignore)
        out['input_ids'].append(row)
        out['labels'].append(lab)
    return {k: np.array(v, np.int64).reshape(-1, L) for k, v in out.items()}, events
