"""Test helper: the Python restatement of the rendered parquet rows (' '.join of vocab strings,
np.save bytes of the masked positions), shared by the render tests."""
import io

import numpy as np


def py_rows(pairs, vocab, order=None):
    """The reference's instance dicts (pretrain.py:345-358) from oracle/GPU pair arrays."""
    rows = []
    n = len(pairs['len_a'])
    for q in (range(n) if order is None else order):
        t = pairs['tokens'][pairs['tok_off'][q]:pairs['tok_off'][q + 1]]
        na = pairs['len_a'][q]
        d = {'A': ' '.join(vocab[i] for i in t[:na]), 'B': ' '.join(vocab[i] for i in t[na:]),
             'is_random_next': bool(pairs['is_random_next'][q]),
             'num_tokens': int(len(t) + 3)}
        if 'pos' in pairs:
            p0, p1 = pairs['pos_off'][q], pairs['pos_off'][q + 1]
            buf = io.BytesIO()
            np.save(buf, np.asarray(pairs['pos'][p0:p1], np.uint16))
            d['masked_lm_positions'] = buf.getvalue()
            d['masked_lm_labels'] = ' '.join(vocab[i] for i in pairs['labels'][p0:p1])
        rows.append(d)
    return rows
