"""Trains tests/golden/unigram_synth.model, the synthetic SentencePiece unigram model of the
tests and of tools/unigram_bench.py, with the `sentencepiece` package: unigram,
the `identity` normaliser, about 2,000 pieces, the sentences of a fixed `lddl_amd.synth` corpus,
one thread, <pad> </s> <unk> <s> as ids 0 to 3 and <mask> as a control symbol. Run once; the
product path never imports this file.

    python tools/unigram_synth.py [--out tests/golden/unigram_synth.model]
"""
import argparse
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'unigram_synth.model'))
    ap.add_argument('--bytes', type=int, default=4 << 20)
    ap.add_argument('--vocab', type=int, default=2000)
    ap.add_argument('--coverage', type=float, default=0.99)
    a = ap.parse_args()
    import sentencepiece as spm
    from lddl_amd import synth
    corp = synth.generate(seed=4321, n_bytes=a.bytes, nonascii_frac=0.05, threads=1)
    text, so = corp.text.tobytes(), corp.sent_off
    sents = (text[so[i]:so[i + 1]].decode('utf-8', 'replace').strip() for i in range(corp.n_sent))
    model = io.BytesIO()
    spm.SentencePieceTrainer.train(
        sentence_iterator=(s for s in sents if s), model_writer=model, vocab_size=a.vocab,
        model_type='unigram', normalization_rule_name='identity', character_coverage=a.coverage,
        num_threads=1, pad_id=0, eos_id=1, unk_id=2, bos_id=3, control_symbols=['<mask>'],
        max_sentencepiece_length=16, hard_vocab_limit=False)
    with open(a.out, 'wb') as f:
        f.write(model.getvalue())
    print(a.out, len(model.getvalue()), 'bytes')


if __name__ == '__main__':
    main()
