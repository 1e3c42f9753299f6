"""The GPT stream as include/lddl_amd.h states it, written sequentially in plain
Python: build the stream as one list, slice rows from it, walk each row. Shares only
denoise_oracle.philox with the other oracles and no code with the product."""
from denoise_oracle import philox

LEN_MASK = (1 << 30) - 1


def fixed(rate):
    return int(rate * 65536 + 0.5)


def doc_tokens(table, d):
    ids, sent_off, sent_len, dso = table
    return [int(v) for s in range(dso[d], dso[d + 1])
            for v in ids[sent_off[s]:sent_off[s] + (int(sent_len[s]) & LEN_MASK)]]


def fim_draw(d, t, fim):
    """None, or (spm, a, b) of document d with t tokens under fim = (rate, spm_rate, seed,
    counter)."""
    if fim is None or t < 1:
        return None
    r = philox(d, fim[3], fim[2])
    if (r[0] >> 16) >= fixed(fim[0]):
        return None
    a, b = sorted(((r[2] * (t + 1)) >> 32, (r[3] * (t + 1)) >> 32))
    return (r[1] >> 16) < fixed(fim[1]), a, b


def layout(tok, draw, pre, mid, suf):
    if draw is None:
        return list(tok)
    spm, a, b = draw
    if spm:
        return [pre, suf] + tok[b:] + [mid] + tok[:a] + tok[a:b]
    return [pre] + tok[:a] + [suf] + tok[b:] + [mid] + tok[a:b]


def stream(table, order=None, fim=None, eos=0, pre=0, mid=0, suf=0):
    """(tokens, terminator flags) of the whole stream, and the draw of every document by id."""
    n_doc = len(table[3]) - 1
    toks, term, draws = [], [], {}
    for d in (range(n_doc) if order is None else order):
        d = int(d)
        tok = doc_tokens(table, d)
        draws[d] = fim_draw(d, len(tok), fim)
        out = layout(tok, draws[d], pre, mid, suf) + [eos]
        toks += out
        term += [False] * (len(out) - 1) + [True]
    return toks, term, draws


def n_rows(total, L):
    return max(0, (total - 1) // L)


def collate(toks, term, L, rows=None, eod_mask_loss=False, reset_position_ids=True, ignore=-100,
            max_seqs=None):
    """The batch as lists: input_ids, labels, position_ids, sequence_ids [B][L], cu_seqlens
    [max_seqs + 1] and n_seqs."""
    rows = range(n_rows(len(toks), L)) if rows is None else rows
    out = {k: [] for k in ('input_ids', 'labels', 'position_ids', 'sequence_ids')}
    starts = []
    for i, r in enumerate(rows):
        w, e = toks[r * L:r * L + L + 1], term[r * L:r * L + L + 1]
        assert len(w) == L + 1
        start, seq, row = 0, 0, {k: [] for k in out}
        for y in range(L):
            if y == 0 or e[y - 1]:
                starts.append(i * L + y)
                start = y
            row['input_ids'].append(w[y])
            row['labels'].append(ignore if eod_mask_loss and e[y] else w[y + 1])
            row['position_ids'].append(y - start if reset_position_ids else y)
            row['sequence_ids'].append(seq)
            seq += e[y]
        for k in out:
            out[k].append(row[k])
    B = len(out['input_ids'])
    max_seqs = len(starts) if max_seqs is None else max_seqs
    kept = starts[:max_seqs]
    out['cu_seqlens'] = kept + [B * L] * (max_seqs + 1 - len(kept))
    out['n_seqs'] = len(starts)
    return out
