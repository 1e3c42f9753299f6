"""Hand-built token tables for the pair stage: sentences of exactly the lengths and ids a test
wants, in the layout `lddl_tokenize` hands to `lddl_pairs_plan` (no text, no tokenizer), with
the compacted tables the oracles take, the case matrix of test_pairs_edges_gpu.py, and the shape
classes a case has to reach for its comparison to mean something (test_pair_tables_host.py
asserts them on the oracle's output, the GPU test again on the device's)."""
import functools
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(REPO, 'lddl_amd', 'assets', 'vocab_synth_uncased_30522.txt')

LEN_HAS_CLS_SEP = 1 << 30     # sent_len flag: the sentence holds a literal [CLS] / [SEP]
SLACK = 0x7FFFFFFF            # what the ids between a sentence's pieces and the next sentence hold
MAX_SENT = 512                # the tokenizer emits at most this many pieces per sentence
PASS_LENS = (127, 128, 129, 255, 256, 257)  # around the gather's 128-token passes
VOCAB_2B, VOCAB_4B = 65534, 65535           # largest 2-byte vocab, smallest 4-byte vocab
DUP = 3
NATIVE_SEED = 987654321


@functools.lru_cache(maxsize=None)
def _vocab_lines():
    with open(VOCAB) as f:
        return tuple(f.read().splitlines())


@functools.lru_cache(maxsize=None)
def special_ids():
    """([CLS], [SEP], [MASK]) ids of the synthetic vocab (unchanged by write_vocab's padding)."""
    lines = _vocab_lines()
    return tuple(lines.index(t) for t in ('[CLS]', '[SEP]', '[MASK]'))


def write_vocab(path, n_lines):
    """The synthetic vocab padded to exactly n_lines lines with bracketed entries."""
    lines = list(_vocab_lines())
    assert n_lines >= len(lines)
    lines += ['[extra{}]'.format(i) for i in range(n_lines - len(lines))]
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return str(path)


def _documents(seq, rng, long):
    """Documents as lists of sentence token counts; the first and the last have two sentences
    that fit one pair, so a pair's A starts at kept token 0 and a pair's B ends at the last."""
    t0 = min(seq - 3, 2 * MAX_SENT)
    docs = [[1] * 40, [1], [512, 512, 512], list(range(1, 18)) * 3]
    for t in dict.fromkeys((2, 3) + PASS_LENS + (seq - 4, seq - 3, seq - 2)):
        if t < 2:
            continue
        for a in sorted({1, t // 2, t - 1}):
            if 1 <= a < t and a <= MAX_SENT and t - a <= MAX_SENT:
                docs.append([a, t - a])
    for _ in range(12):
        docs.append([int(x) for x in rng.integers(1, 40, size=int(rng.integers(1, 12)))])
    if long:
        docs.append([512] * 20)
        docs.append([500, 1, 512, 7] + [512] * 8 + [3])
    docs = [docs[i] for i in rng.permutation(len(docs))]
    return [[t0 // 2, t0 - t0 // 2]] + docs + [[t0 - t0 // 2, t0 // 2]]


def build(seq, vocab_size, seed, long=False):
    """A hand-built batch as numpy arrays.

    Device side (make_pairs / lddl_pairs_plan): sent_off, ids, sent_len, doc_sent_off,
    part_doc_off (three partitions, the middle one without documents). Sentence s's tokens are
    ids[sent_off[s] + i], every stride is larger than the sentence, the slack holds SLACK;
    zero-length sentences and documents made only of them lie between the real ones, one at the
    very front and one at the very end.

    Oracle side: k_ids / k_off (kept tokens and the kept sentences' offsets), k_doc (kept
    documents' kept-sentence offsets), kp_off (kept-document range of each partition), derived
    as the reference filters (_get_documents: empty sentences, then empty documents)."""
    rng = np.random.default_rng(seed)
    cls_id, sep_id, mask_id = special_ids()
    docs = _documents(seq, rng, long)
    raw = [[0, 0]]
    for d in docs:
        d = list(d)
        if rng.random() < 0.3:
            for _ in range(int(rng.integers(1, 4))):
                d.insert(int(rng.integers(0, len(d) + 1)), 0)
        raw.append(d)
        if rng.random() < 0.2:
            raw.append([0] * int(rng.integers(1, 4)))
    raw.append([0])
    lens = np.asarray([n for d in raw for n in d], np.int64)
    assert lens.max() <= MAX_SENT
    doc_sent_off = np.concatenate([[0], np.cumsum([len(d) for d in raw])]).astype(np.int64)
    sent_off = np.concatenate([[0], np.cumsum(lens + rng.integers(1, 4, size=len(lens)))]).astype(np.int64)
    total = int(lens.sum())
    k_ids = rng.integers(1000, vocab_size, size=total).astype(np.int32)
    r = rng.random(total)
    k_ids[r < 0.02] = vocab_size - 1
    k_ids[(r >= 0.02) & (r < 0.03)] = cls_id
    k_ids[(r >= 0.03) & (r < 0.04)] = sep_id
    tok_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.full(int(sent_off[-1]), SLACK, np.int32)
    sent_len = lens.astype(np.int32)
    for s in range(len(lens)):
        t = k_ids[tok_start[s]:tok_start[s + 1]]
        ids[sent_off[s]:sent_off[s] + len(t)] = t
        if ((t == cls_id) | (t == sep_id)).any():
            sent_len[s] |= LEN_HAS_CLS_SEP
    half = len(raw) // 2
    part_doc_off = np.asarray([0, half, half, len(raw)], np.int64)
    # the reference drops empty sentences and then empty documents before pairing
    kept = [[s for s in range(doc_sent_off[d], doc_sent_off[d + 1]) if lens[s] > 0]
            for d in range(len(raw))]
    is_kept = np.asarray([len(d) > 0 for d in kept])
    k_doc = np.concatenate([[0], np.cumsum([len(d) for d in kept if d])]).astype(np.int64)
    k_off = np.concatenate([[0], np.cumsum(lens[lens > 0])]).astype(np.int64)
    kd_pos = np.concatenate([[0], np.cumsum(is_kept)]).astype(np.int64)
    return dict(sent_off=sent_off, ids=ids, sent_len=sent_len, doc_sent_off=doc_sent_off,
                part_doc_off=part_doc_off, k_ids=k_ids, k_off=k_off, k_doc=k_doc,
                kp_off=kd_pos[part_doc_off], vocab_size=vocab_size, cls_id=cls_id, sep_id=sep_id,
                mask_id=mask_id, first_len=docs[0][0], last_len=docs[-1][-1])


# ---------------------------------------------------------------------------------------------
# The case matrix ("Pair-stage edge cases"). ratio None: masking=False.
# ---------------------------------------------------------------------------------------------
class Case:
    def __init__(self, rng, vocab_size, seq, ratio, long=False, seeds=None):
        self.rng, self.vocab_size, self.seq, self.ratio, self.long = rng, vocab_size, seq, ratio, long
        self.masking = ratio is not None
        self.id = '{}-{}B-s{}-{}'.format(rng, 2 if vocab_size <= VOCAB_2B else 4, seq,
                                         'nomask' if ratio is None else 'r{}'.format(ratio))
        self.data_seed, seed0 = seeds or SEEDS[self.id]
        self.part_seed = np.asarray([seed0, seed0 + 1, seed0 + 2], np.int64)

    def tables(self):
        return _tables(self.seq, self.vocab_size, self.data_seed, self.long)

    def oracle(self):
        """The oracle's output of every partition (None for a partition without documents)."""
        from oracle import oracle as O
        t = self.tables()
        out = []
        for p in range(len(self.part_seed)):
            ds = t['k_doc'][t['kp_off'][p]:t['kp_off'][p + 1] + 1]
            if len(ds) < 2:
                out.append(None)
                continue
            tail = (DUP, self.seq, self.masking, t['vocab_size'], t['cls_id'], t['sep_id'], t['mask_id'])
            kw = dict(masked_lm_ratio=self.ratio) if self.masking else {}
            if self.rng == 'replay':
                out.append(O.partition_pairs(ds, t['k_off'], t['k_ids'], int(self.part_seed[p]), *tail, **kw))
            else:
                out.append(O.partition_pairs_native(ds, t['k_off'], t['k_ids'], NATIVE_SEED,
                                                    int(self.part_seed[p]), *tail, **kw))
        return out


@functools.lru_cache(maxsize=4)
def _tables(seq, vocab_size, data_seed, long):
    t = build(seq, vocab_size, data_seed, long)
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)  # shared between the cases and tests that use them
    return t


def merge(parts):
    """The partitions' oracle outputs as one output dict (the form PairBatch.to_host() has)."""
    parts = [p for p in parts if p is not None]
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0] if not k.endswith('_off')}
    for k in ('tok_off', 'pos_off'):
        if k in parts[0]:
            out[k] = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(p[k]) for p in parts]))])
    return out


def classes(out, seq, tab, ratio=None):
    """Which shape classes occur in an output dict (the oracle's, merged, or the device's):
    {name: bool} of every class that applies to the case."""
    na = np.asarray(out['len_a']).astype(np.int64)
    tok_off = np.asarray(out['tok_off']).astype(np.int64)
    n = np.diff(tok_off)
    nb = n - na
    tokens = np.asarray(out['tokens']).astype(np.int64)
    top = tab['vocab_size'] - 1
    c = {'len(A) == 1': (na == 1).any(), 'len(B) == 1': (nb == 1).any(), 'n == 2': (n == 2).any(),
         'n == seq - 3': (n == seq - 3).any()}
    for k in range(8):
        c['len(A) % 8 == {}'.format(k)] = (na % 8 == k).any()
    for t in PASS_LENS:
        if t <= seq - 3:
            c['n == {}'.format(t)] = (n == t).any()
    orig = tokens.copy()
    if 'pos' in out:
        pos = np.asarray(out['pos']).astype(np.int64)
        lab = np.asarray(out['labels']).astype(np.int64)
        q = np.repeat(np.arange(len(na)), np.diff(np.asarray(out['pos_off']).astype(np.int64)))
        x = np.where(pos <= na[q], pos - 1, pos - 2)  # the masked token's place in A + B
        c['mask at 1'] = (pos == 1).any()
        c['mask at len(A)'] = (pos == na[q]).any()
        c['mask at len(A) + 2'] = (pos == na[q] + 2).any()
        c['mask at n + 1'] = (pos == n[q] + 1).any()
        c['random replacement == top id'] = ((tokens[tok_off[q] + x] == top) & (lab != top)).any()
        orig[tok_off[q] + x] = lab
        if ratio == 1.0 and seq - 3 >= 128:
            n_pass = (seq + 127) // 128
            full = np.bincount(q * n_pass + x // 128, minlength=len(na) * n_pass) == 128
            c['a pass with all 128 tokens masked'] = full.any()
    dense = tab['k_ids'].astype(np.int64)
    l0, l1 = tab['first_len'], tab['last_len']
    # A is the whole first kept sentence / B is the whole last one: with ids drawn from
    # > 64,000 values no other window of that length (>= 8 tokens) looks the same
    c['a pair starts at kept token 0'] = any(
        np.array_equal(orig[tok_off[i]:tok_off[i] + l0], dense[:l0]) for i in np.flatnonzero(na == l0))
    c['a pair ends at the last kept token'] = any(
        np.array_equal(orig[tok_off[i + 1] - l1:tok_off[i + 1]], dense[-l1:]) for i in np.flatnonzero(nb == l1))
    return {k: bool(v) for k, v in c.items()}


def missing(out, seq, tab, ratio=None):
    return [k for k, v in classes(out, seq, tab, ratio).items() if not v]


# (data seed, first partition seed) of every case, searched so that the oracle's output reaches
# every class of the case: all but one are reached by nearly every seed, but a random
# replacement is the top id once in vocab_size draws, a few hundred of which a case makes.
SEEDS = {
    'replay-2B-s20-r0.15': (1, 3346),
    'replay-2B-s131-r0.15': (1, 328),
    'replay-2B-s132-r0.15': (1, 946),
    'replay-2B-s260-r0.15': (1, 877),
    'replay-2B-s512-r0.15': (1, 136),
    'replay-2B-s132-r1.0': (1, 145),
    'replay-2B-s512-r1.0': (1, 136),
    'native-2B-s20-r0.15': (1, 964),
    'native-2B-s131-r0.15': (1, 454),
    'native-2B-s132-r0.15': (1, 415),
    'native-2B-s260-r0.15': (1, 415),
    'native-2B-s512-r0.15': (1, 355),
    'native-2B-s132-r1.0': (1, 121),
    'native-2B-s512-r1.0': (1, 103),
    'native-2B-s600-r0.15': (1, 415),
    'replay-2B-s132-nomask': (1, 100),
    'native-2B-s601-r0.15': (1, 121),
    'native-2B-s1024-r0.15': (1, 121),
    'native-2B-s4096-r0.15': (1, 487),
    'replay-4B-s20-r0.15': (1, 559),
    'replay-4B-s131-r0.15': (1, 1786),
    'replay-4B-s132-r0.15': (1, 898),
    'replay-4B-s260-r0.15': (1, 277),
    'replay-4B-s512-r0.15': (1, 181),
    'replay-4B-s132-r1.0': (1, 181),
    'replay-4B-s512-r1.0': (1, 127),
    'native-4B-s20-r0.15': (1, 964),
    'native-4B-s131-r0.15': (1, 454),
    'native-4B-s132-r0.15': (1, 415),
    'native-4B-s260-r0.15': (1, 415),
    'native-4B-s512-r0.15': (1, 355),
    'native-4B-s132-r1.0': (1, 121),
    'native-4B-s512-r1.0': (1, 103),
    'native-4B-s600-r0.15': (1, 415),
    'replay-4B-s132-nomask': (1, 100),
    'native-4B-s601-r0.15': (1, 121),
    'native-4B-s1024-r0.15': (1, 121),
    'native-4B-s4096-r0.15': (1, 487),
}


def _case_list(seeds=None):
    out = []
    for v in (VOCAB_2B, VOCAB_4B):
        for rng in ('replay', 'native'):
            out += [Case(rng, v, s, 0.15, seeds=seeds) for s in (20, 131, 132, 260, 512)]
            out += [Case(rng, v, s, 1.0, seeds=seeds) for s in (132, 512)]
        out.append(Case('native', v, 600, 0.15, seeds=seeds))
        out.append(Case('replay', v, 132, None, seeds=seeds))
        out += [Case('native', v, s, 0.15, long=True, seeds=seeds) for s in (601, 1024, 4096)]
    return out


CASES = _case_list() if SEEDS else []
