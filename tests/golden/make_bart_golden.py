"""Golden fixture for the BART preprocessor (tests/golden/bart.json), made by the REFERENCE's own
`_get_sequences` and `save` (lddl/dask/bart/pretrain.py:41-153) in the dev container
(/root/reference does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_bart_golden.py

A small corpus directory (wikipedia/en/*.txt, books/*.txt) is written to a temporary directory:
`<id> <text>` lines cut from the documents of make_goldens.make_doc_lines, hand-written lines with Unicode whitespace
inside sentences, blank lines, lines with surrounding whitespace, and one article of more than
200 sentences. Under dask's synchronous scheduler, for --target-seq-length in {3, 11, 35, 128,
512} and two block sizes (the smaller one cuts the long article into blocks, some of which hold
no line start: empty partitions), the reference's bag is computed partition by partition and its
`save(..., 'txt')` writes the text files. Recorded:

  * files: the input files (path relative to the corpus root -> text);
  * args: the reference parser's options (names, defaults, choices);
  * cases: target_seq_length, block_size, the chunk strings of every partition and the exact
    content of every txt file, plus the file names of the parquet directory.

Parquet: `save(..., 'parquet')` goes through dask.dataframe, which does not import with the
NumPy / pandas of this container (make_goldens.import_reference stubs it). The rows of
part.<i>.parquet are the `sentences` of partition i, which is what `partitions` holds; the file
names recorded are those of dask 2021.10's to_parquet(write_index=False) (one part.<i>.parquet per
partition, `_common_metadata`, `_metadata`).

nltk's English model is not available offline: `sent_tokenize` is the untrained
PunktSentenceTokenizer (import_reference), which is `PunktParams()` here.
Import recipe: make_goldens.import_reference. Only data is written.
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_goldens as G  # noqa: E402

TARGETS = (3, 11, 35, 128, 512)
BLOCK_SIZES = (1000, 6000)

HAND = [
    'hand-0 Alpha\u00a0beta gamma delta. Epsilon\u3000zeta eta theta! Iota\x1ckappa\x1flambda?',
    '',
    '   \t hand-1 Surrounded by blanks. Still one article.  \u00a0 ',
    '\u3000hand-2 starts after an ideographic space.\x0b Vertical tab and form feed\x0c follow. End',
    '  ',
    'hand-3\u0085next-line is whitespace too.    A b c d e f g h i j k l m.',
    'hand-4 éè 中文 \U0001f600\U0001f601 mixed-width wörds. 中 文! \U0001f600 \U0001f601?',
    'hand-5 Zero\u200bwidth\u200bspace is no whitespace. Nor\u2060is\ufeffthis. Nor\u180ethat.',
    ' ',
    'hand-6 x',
    'hand-7 "Quoted end." (Bracketed.) Next one... and on. A.B. Smith went. 3.5 is a number.',
]


def long_article():
    sents = []
    for k in range(210):
        n = 1 + (k * 7) % 4
        sents.append(' '.join('a{}'.format((k + j) % 10) for j in range(n)).capitalize() + '.?!'[k % 3])
    return 'long-0 ' + '  '.join(sents)


def doc_lines():
    """The documents of make_goldens.make_doc_lines cut into short `<id> <text>` articles of a
    few sentences each (the fixture holds every case's output twice, so the corpus is kept to a
    few KB); the 600-word sentence is cut to 140 words, still more than a chunk of 128."""
    lines = []
    for d, line in enumerate(G.make_doc_lines(2000, 4242, 0.05)):
        doc_id, _, text = line.partition(' ')
        if doc_id == 'edge-4':
            text = ' '.join(['plut'] * 140) + '. Short after.'
        piece, k = '', 0
        for sent in text.split('. '):
            piece += sent + '. '
            if len(piece) > 60 + 17 * (k % 5):
                lines.append('{}.{} {}'.format(doc_id, k, piece.rstrip().rstrip('.') + '.'))
                piece, k = '', k + 1
        if piece.strip('. '):
            lines.append('{}.{} {}'.format(doc_id, k, piece.rstrip().rstrip('.') + '.'))
    return lines


def write_corpus(root):
    lines = doc_lines()
    third = len(lines) // 3
    files = {
        'wikipedia/en/a.txt': lines[:third] + HAND[:6],
        'wikipedia/en/b.txt': HAND[6:] + [long_article()] + lines[third:2 * third],
        'books/c.txt': lines[2 * third:] + ['', 'tail-0 The last line has no newline after it.'],
    }
    out = {}
    for rel, ls in files.items():
        fn = os.path.join(root, rel)
        os.makedirs(os.path.dirname(fn), exist_ok=True)
        text = '\n'.join(ls) + ('' if rel.startswith('books') else '\n')
        with open(fn, 'w', encoding='utf-8', newline='') as f:
            f.write(text)
        out[rel] = text
    print('corpus: {} lines, {} bytes'.format(sum(len(ls) for ls in files.values()),
                                              sum(len(t.encode('utf-8')) for t in out.values())))
    return out


def parser_options(parser):
    opts = {}
    for a in parser._actions:
        if not a.option_strings or a.dest == 'help':
            continue
        default = a.default
        if a.dest == 'local_n_workers':
            default = 'os.cpu_count()'  # lddl/dask/bart/pretrain.py:199
        opts[a.option_strings[0]] = dict(dest=a.dest, default=default, required=bool(a.required),
                                         choices=None if a.choices is None else list(a.choices))
    return opts


def main():
    G.import_reference()
    import argparse
    import dask
    from lddl.dask.bart import pretrain as bart
    gold = {'args': parser_options(bart.attach_args(argparse.ArgumentParser())), 'cases': []}
    with tempfile.TemporaryDirectory() as root, dask.config.set(scheduler='synchronous'):
        gold['files'] = write_corpus(root)
        for bs in BLOCK_SIZES:
            for target in TARGETS:
                def seqs():
                    return bart._get_sequences(wikipedia_path=os.path.join(root, 'wikipedia'),
                                               books_path=os.path.join(root, 'books'),
                                               target_seq_length=target, blocksize=bs)
                parts = [[r['sentences'] for r in d.compute()] for d in seqs().to_delayed()]
                with tempfile.TemporaryDirectory() as sink:
                    bart.save(seqs(), sink, output_format='txt')
                    txt = {}
                    for fn in sorted(os.listdir(sink)):
                        with open(os.path.join(sink, fn), 'rb') as f:
                            txt[fn] = f.read().decode('utf-8')
                pq_files = ['part.{}.parquet'.format(i) for i in range(len(parts))] + \
                    ['_common_metadata', '_metadata']
                gold['cases'].append(dict(target_seq_length=target, block_size=bs, partitions=parts,
                                          txt=txt, parquet_files=sorted(pq_files)))
                print('bs {} target {}: {} partitions ({} empty), {} chunks, {} txt files'.format(
                    bs, target, len(parts), sum(1 for p in parts if not p),
                    sum(map(len, parts)), len(txt)))
    out = os.path.join(HERE, 'bart.json')
    with open(out, 'w', encoding='utf-8') as f:
        json.dump(gold, f, ensure_ascii=False, separators=(',', ':'))
        f.write('\n')
    print(out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
