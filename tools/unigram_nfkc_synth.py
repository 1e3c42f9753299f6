"""Trains tests/golden/unigram_nfkc.model, the synthetic SentencePiece unigram model with the
full `nmt_nfkc` character map and byte fallback, with the `sentencepiece` package:
tools/unigram_synth.py's corpus and settings, about 1,000 pieces. Prints the map's key count,
longest key and largest growth as `lddl_amd.unigram.load_normalizer` reads them. Run once; the
product path never imports this file.

    python tools/unigram_nfkc_synth.py [--out tests/golden/unigram_nfkc.model]
"""
import argparse
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'unigram_nfkc.model'))
    ap.add_argument('--bytes', type=int, default=2 << 20)
    ap.add_argument('--vocab', type=int, default=1000)
    ap.add_argument('--coverage', type=float, default=0.99)
    a = ap.parse_args()
    import sentencepiece as spm
    from lddl_amd import synth, unigram
    corp = synth.generate(seed=4321, n_bytes=a.bytes, nonascii_frac=0.05, threads=1)
    text, so = corp.text.tobytes(), corp.sent_off
    sents = (text[so[i]:so[i + 1]].decode('utf-8', 'replace').strip() for i in range(corp.n_sent))
    model = io.BytesIO()
    spm.SentencePieceTrainer.train(
        sentence_iterator=(s for s in sents if s), model_writer=model, vocab_size=a.vocab,
        model_type='unigram', normalization_rule_name='nmt_nfkc', byte_fallback=True,
        character_coverage=a.coverage, num_threads=1, pad_id=0, eos_id=1, unk_id=2, bos_id=3,
        control_symbols=['<mask>'], max_sentencepiece_length=16, hard_vocab_limit=False)
    with open(a.out, 'wb') as f:
        f.write(model.getvalue())
    print(a.out, len(model.getvalue()), 'bytes')
    keys, repls, byte_pieces = unigram.load_normalizer(a.out)
    grow = max(zip(keys, repls), key=lambda kr: len(kr[1]) / len(kr[0]))
    print('rules', len(keys), 'longest key', max(map(len, keys)), 'longest replacement',
          max(map(len, repls)), 'largest growth', len(grow[0]), '->', len(grow[1]), 'bytes',
          'byte pieces', byte_pieces is not None)


if __name__ == '__main__':
    main()
