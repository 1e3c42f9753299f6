"""Hand-made inputs of the model-parallel loader tests, shared by tests/test_loader_mp.py and
the golden generator (tests/golden/make_loader_mp_golden.py).

Collate cases: static-masking batches for `_to_encoded_inputs` of lddl.torch_mp, chosen for the
collate kernel's edges (one wave per sample, four waves per workgroup, 64-lane strides over the
row and over the positions)."""
import io
import random

import numpy as np

# arguments of the world-4 raw-order run (two data-parallel groups of two ranks)
MP_WORLD = 4
MP_SHARDS = 8
MP_RAW_KWARGS = dict(shuffle_buffer_size=8, shuffle_buffer_warmup_factor=2, base_seed=777,
                     start_epoch=1, return_raw_samples=True)
MP_RAW_DL_KWARGS = {'batch_size': 3, 'num_workers': 2}
# arguments of the world-1 binned static run (those of the binned golden in loader.npz)
MP_BIN_KWARGS = dict(local_rank=0, dp_rank=0, shuffle_buffer_size=8,
                     shuffle_buffer_warmup_factor=2, base_seed=4242)
MP_BIN_DL_KWARGS = {'batch_size': 3, 'num_workers': 2}
MP_KEYS = ('input_ids', 'token_type_ids', 'attention_mask', 'labels', 'masked_lm_positions',
           'next_sentence_labels')
ABSENT = 'zzzznotaword'  # in no vocab: convert_tokens_to_ids gives [UNK]


def raw_lines(batch):
    """One raw (return_raw_samples=True) batch as comparable strings."""
    return ['{}|{}|{}'.format(a, b, int(c)) for a, b, c in zip(*batch[:3])] + ['--batch--']


def _npy(a):
    b = io.BytesIO()
    np.save(b, np.asarray(a, np.uint16))
    return b.getvalue()


def _sample(rng, words, na, nb, pos, absent_at=()):
    """(A, B, is_random_next, masked_lm_positions, masked_lm_labels). The label of a position is
    the token there, or a random word at a special or padding slot; equal positions get equal
    labels (an indexed assignment with duplicate indices is defined only then). The k-th label
    for k in absent_at is a token outside the vocab."""
    A = [rng.choice(words) for _ in range(na)]
    B = [rng.choice(words) for _ in range(nb)]
    seq = ['[CLS]'] + A + ['[SEP]'] + B + ['[SEP]']
    by_pos = {}
    labels = []
    for k, p in enumerate(pos):
        if p not in by_pos:
            by_pos[p] = seq[p] if p < len(seq) and not seq[p].startswith('[') else rng.choice(words)
        labels.append(ABSENT if k in absent_at else by_pos[p])
    return (' '.join(A), ' '.join(B), rng.random() < 0.5, _npy(pos), ' '.join(labels))


def make_collate_cases(vocab_file):
    """[(name, batch, sequence_length_alignment, ignore_index)]."""
    with open(vocab_file, encoding='utf-8') as f:
        vocab = [l.rstrip('\n') for l in f]
    words = [w for w in vocab[1000:6000] if not w.startswith('[')]
    rng = random.Random(11)
    cases = []
    # B = 1; end = 9, L = 16: position 0, na + 1, end - 1, a padding slot and L - 1
    cases.append(('b1', [_sample(rng, words, 3, 3, [0, 4, 8, 10, 15])], 8, -1))
    # B = 5: the second workgroup has one active wave of four; end = 21 -> L = 32. A sample with
    # no positions, duplicate positions, a label outside the vocab, the same edges as above
    cases.append(('b5', [
        _sample(rng, words, 5, 7, [2, 9]),
        _sample(rng, words, 1, 1, []),
        _sample(rng, words, 9, 9, [3, 3, 7, 12, 12, 12], absent_at=(2,)),
        _sample(rng, words, 2, 6, [0, 3, 10, 20, 31], absent_at=(1,)),
        _sample(rng, words, 4, 3, [5]),
    ], 16, -100))
    # na + nb + 3 = 65 with alignment 1: L = 65, two 64-lane strides, the second of one slot
    cases.append(('s65', [
        _sample(rng, words, 30, 32, [0, 31, 63, 64]),
        _sample(rng, words, 7, 2, [1, 8, 11, 40, 64]),
    ], 1, -1))
    # the same rows aligned to 8 and 16 (L = 72, 80) and with the other ignore_index
    cases.append(('s65a8', cases[-1][1], 8, -100))
    cases.append(('s65a16', cases[-1][1], 16, -1))
    # na + nb + 3 = 130: three strides (L = 136 at alignment 8, 130 at 1); 70 positions, more than
    # one stride of the marking loop, with duplicates across the strides
    many = sorted(rng.sample(range(1, 129), 66) + [5, 5, 100, 127])
    many = [p for p in many if p != 61]  # 61 is na + 1: added below, explicitly
    cases.append(('s130', [
        _sample(rng, words, 60, 67, [0, 61] + many + [129, 130, 135]),
        _sample(rng, words, 12, 1, [13, 15, 16, 135]),
        _sample(rng, words, 64, 63, [64, 65, 66, 128, 129]),
    ], 8, -100))
    cases.append(('s130a1', [
        _sample(rng, words, 1, 126, [0, 2, 63, 64, 127, 128, 129], absent_at=(3,)),
        _sample(rng, words, 20, 20, []),
    ], 1, -1))
    return cases
