"""T5 span corruption without a GPU: the widths against the oracle's formulas, the
refusals of both entry points, the Python argument errors, and the oracle's own invariants."""
import pytest

import t5_oracle as O

CONFIGS = [(0.15, 3.0, 100), (0.5, 1.0, 256), (0.99, 64.0, 3)]
DEF = O.fixed(*CONFIGS[0])
# (seed, counter, n) at the defaults, row 0: the non-noise keys of rank k - 1 and k are equal,
# so the position decides. Found by counting seeds up from 1 with the oracle's keys on the CPU.
TIE = (71422, 0, 500)
KW = dict(sentinel_first=1099, eos=2, pad=1, dec_start=1, ignore=-100)


@pytest.mark.parametrize('cfg', CONFIGS)
def test_lengths_are_the_oracles_and_do_not_decrease(cfg):
    from lddl_amd.torch import t5_lengths, t5_tokens_length
    got = [t5_lengths(n, *cfg) for n in range(1, 601)]
    assert got == [O.lengths(n, *O.fixed(*cfg)) for n in range(1, 601)]
    assert all(a[0] <= b[0] and a[1] <= b[1] for a, b in zip(got, got[1:]))
    for width in (2, 3, 17, 128, 512):  # t5_tokens_length is the inverse
        t = t5_tokens_length(width, *cfg)
        assert t5_lengths(t, *cfg)[0] <= width < t5_lengths(t + 1, *cfg)[0]


@pytest.mark.parametrize('bad', [
    dict(L=2), dict(L=(1 << 24) + 1), dict(in_len=0), dict(in_len=(1 << 24) + 1), dict(tgt_len=0),
    dict(tgt_len=(1 << 24) + 1), dict(dq=0), dict(dq=65536), dict(iq=0), dict(iq=65537),
    dict(ns=0), dict(ns=257), dict(first=98), dict()])
def test_both_entry_points_refuse(bad):
    """With NULL pointers everywhere: a bad value is refused before the pointers are looked at,
    good values with batch > 0 fail on the pointers, and batch = 0 returns 0."""
    from lddl_amd._native import lib
    a = dict(dict(L=130, in_len=120, tgt_len=40, dq=DEF[0], iq=DEF[1], ns=100, first=1099), **bad)
    call = lambda batch: lib.lddl_t5_corrupt(  # noqa: E731
        None, None, None, None, None, None, None, batch, a['L'], a['in_len'], a['tgt_len'],
        a['dq'], a['iq'], a['ns'], a['first'], 2, 1, 1, -100, 5, 6, *[None] * 6)
    assert call(4) == -1 and ('null' in lib.lddl_last_error().decode()) == (not bad)
    assert call(0) == (-1 if bad else 0)
    if not {'in_len', 'tgt_len', 'first'} & set(bad):
        assert lib.lddl_t5_lengths(a['L'] - 2, a['dq'], a['iq'], a['ns'], None, None) == -1
        assert ('null' in lib.lddl_last_error().decode()) == (not bad)


@pytest.mark.parametrize('kw', [
    dict(noise_density=0), dict(noise_density=1.0), dict(noise_density='a'),
    dict(mean_noise_span_length=0.5), dict(mean_noise_span_length=float('nan')),
    dict(n_sentinels=0), dict(n_sentinels=257), dict(n_sentinels=2.5), dict(noise=3),
    dict(in_len=0), dict(tgt_len=(1 << 24) + 1), dict(special_ids={'bos_id': 0})])
def test_python_refuses_bad_arguments_before_the_gpu(monkeypatch, tmp_path, kw):
    import lddl_amd.context as C
    from lddl_amd import bpe as B
    from lddl_amd.torch import get_t5_pretrain_data_loader, t5_corrupt

    def boom(*a, **k):
        raise AssertionError('the GPU was touched')
    monkeypatch.setattr(C.Context, '__init__', boom)
    with pytest.raises(ValueError):
        t5_corrupt(None, None, None, **kw)
    if not {'noise', 'in_len', 'tgt_len'} & set(kw):
        (tmp_path / 'a.txt').write_text('One document. Two sentences.\n')
        with pytest.raises(ValueError):
            get_t5_pretrain_data_loader(str(tmp_path), (B.SYNTH_VOCAB, B.SYNTH_MERGES), 4, **kw)


def restore(inp, lab, first, k):
    """The clean row (no eos), each sentinel replaced by the target's run behind the same one."""
    sent = set(range(first - k + 1, first + 1))
    cuts = [j for j, v in enumerate(lab) if v in sent] + [len(lab)]
    run = {lab[a]: lab[a + 1:b] for a, b in zip(cuts, cuts[1:])}
    return [x for v in inp for x in (run[v] if v in sent else [v])]


@pytest.mark.parametrize('n,cfg', [(1, 0), (2, 0), (65, 0), (130, 1), (500, 0), (500, 2)])
def test_oracle_rows_hold_exact_counts_and_restore_the_tokens(n, cfg):
    t, q = list(range(10, 10 + n)), O.fixed(*CONFIGS[cfg])
    inp, att, lab, dec, sl, tl, noise = O.corrupt_row(1, t, n + 2, *O.lengths(n, *q), q, seed=9,
                                                      counter=4, **KW)
    N, k = O.counts(n, *q)
    assert (sl, tl) == O.lengths(n, *q) == (sum(att), len(lab)) and sum(noise) == N
    assert sum(1 for a, b in zip([0] + noise, noise) if b and not a) == k  # the spans
    assert n < 2 or (noise[0] == 0 and noise[-1] == 1)
    assert restore(inp[:-1], lab[:-1], KW['sentinel_first'], k) == t
    assert dec == [KW['dec_start']] + lab[:-1]


def test_the_committed_tie_is_a_tie_at_the_threshold():
    N, k, _, km = O.row_keys(0, TIE[2], 0, DEF, *TIE[:2])
    order = O.ranked(km, TIE[2] - N)
    assert km[order[k - 2] - 1] == km[order[k - 1] - 1] and order[k - 2] < order[k - 1]
