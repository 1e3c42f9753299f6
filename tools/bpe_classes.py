"""Writes lddl_amd/assets/bpe_classes.txt: the character classes of GPT-2's pre-tokenizer
 as ranges of code points, from this interpreter's `unicodedata`. The committed file
was made with Unicode 13.0.0 (its first line says so); the classes a tokenizer uses are the
file's, whatever Python runs it.

  L  \\p{L}: general category L*          S  \\s: the White_Space property (WHITE_SPACE)
  N  \\p{N}: general category N*          everything else, unlisted: "other"

One range a line, `first..last class` in hex. lddl_amd.bpe.load_classes turns the file into the
two-level table lddl_bpe_create takes (include/lddl_amd.h).

    python tools/bpe_classes.py [out]
"""
import os
import sys
import unicodedata

WHITE_SPACE = frozenset([*range(0x09, 0x0E), 0x20, 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B),
                         0x2028, 0x2029, 0x202F, 0x205F, 0x3000])


def char_class(cp):
    if cp in WHITE_SPACE:
        return 'S'
    cat = unicodedata.category(chr(cp))[0]
    return cat if cat in 'LN' else None


def build():
    lines = ['# bpe_classes Unicode {}'.format(unicodedata.unidata_version),
             '# first..last class: L letter (L*), N number (N*), S white space; the rest is other']
    first, cur = 0, None
    for cp in range(0x110001):
        c = char_class(cp) if cp < 0x110000 else None
        if c != cur:
            if cur:
                lines.append('{:04X}..{:04X} {}'.format(first, cp - 1, cur))
            first, cur = cp, c
    return '\n'.join(lines) + '\n'


if __name__ == '__main__':
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'lddl_amd', 'assets',
        'bpe_classes.txt')
    text = build()
    with open(out, 'w') as f:
        f.write(text)
    print('{}: {} ranges, Unicode {}'.format(out, text.count('\n') - 2, unicodedata.unidata_version))
