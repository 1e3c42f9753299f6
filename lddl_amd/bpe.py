"""Byte-level BPE on the device: GPT-2's tokenizer, which RoBERTa and BART
checkpoints share, from `vocab.json` and `merges.txt`. `BpeContext` undoes JSON and GPT-2's
byte-to-unicode map, hands raw byte strings and (left, right, merged) id triples in rank order
to lddl_bpe_create, and wraps lddl_bpe_tokenize (include/lddl_amd.h states the semantics).
pattern='cl100k' / 'qwen2' and ignore_merges=True give the ids of Llama 3, GPT-4,
Qwen2 and DeepSeek checkpoints; `BpeContext.from_tokenizer_json` reads all of it from a Hugging
Face tokenizer.json. Argument errors are raised before the native library is imported.
"""
import json
import os

import numpy as np

ASSETS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'assets')
CLASSES = os.path.join(ASSETS, 'bpe_classes.txt')
SYNTH_VOCAB = os.path.join(ASSETS, 'bpe_synth_vocab.json')
SYNTH_MERGES = os.path.join(ASSETS, 'bpe_synth_merges.txt')
SPECIALS = ('<s>', '<pad>', '</s>', '<unk>', '<mask>')
MAX_WORD = 1024  # LDDL_BPE_MAX_WORD
# pattern -> (lddl_bpe_set_pattern's name, its digit_group when none is given)
PATTERNS = {'gpt2': ('gpt2', 0), 'cl100k': ('cl100k', 3), 'qwen2': ('cl100k', 1)}
_CL = (r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}%s| ?[^\s\p{L}\p{N}]+[\r\n]*"
       r"|\s*[\r\n]+|\s+(?!\S)|\s+")
# the regex strings of a tokenizer.json's Split pre-tokenizer that from_tokenizer_json knows
SPLIT_REGEX = {
    r"'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+": 'gpt2',
    _CL % '{1,3}': 'cl100k',
    _CL % '': 'qwen2',
}


def check_options(pattern='gpt2', digit_group=None, ignore_merges=False):
    """(lddl_bpe_set_pattern's name, digit_group, ignore_merges) of BpeContext's keywords, or a
    ValueError."""
    if pattern not in PATTERNS:
        raise ValueError('pattern must be one of {}, not {!r}'.format(sorted(PATTERNS), pattern))
    name, group = PATTERNS[pattern]
    if digit_group is not None:
        if name == 'gpt2' or isinstance(digit_group, bool) or digit_group not in (1, 3):
            raise ValueError("digit_group is 1 or 3 and goes with pattern='cl100k', not {!r} with "
                             '{!r}'.format(digit_group, pattern))
        group = digit_group
    if not isinstance(ignore_merges, bool):
        raise ValueError('ignore_merges must be a bool, not {!r}'.format(ignore_merges))
    return name, group, ignore_merges


def bytes_to_unicode():
    """GPT-2's map of the 256 byte values to printable characters (encoder.py)."""
    bs = list(range(ord('!'), ord('~') + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {b: chr(c) for b, c in zip(bs, cs)}


def load_tables(vocab_json, merges_txt):
    """(tokens: list of bytes by id, vocab: str -> id, merges: int32 [n, 3]) of the two files;
    FileNotFoundError / ValueError on what cannot be a byte-level BPE vocabulary."""
    for name, f in (('vocab_json', vocab_json), ('merges_txt', merges_txt)):
        if not isinstance(f, str) or not os.path.isfile(f):
            raise FileNotFoundError('{} {!r}: a local file is required'.format(name, f))
    with open(vocab_json, encoding='utf-8') as f:
        try:
            vocab = json.load(f)
        except ValueError as e:
            raise ValueError('{}: not JSON ({})'.format(vocab_json, e)) from None
    if not isinstance(vocab, dict) or not vocab or not all(
            isinstance(k, str) and isinstance(v, int) and not isinstance(v, bool) and v >= 0
            for k, v in vocab.items()):
        raise ValueError('{}: expected an object of token -> id'.format(vocab_json))
    if len(set(vocab.values())) != len(vocab):
        raise ValueError('{}: two tokens share an id'.format(vocab_json))
    u2b = {c: b for b, c in bytes_to_unicode().items()}
    tokens = [b''] * (max(vocab.values()) + 1)
    for t, i in vocab.items():
        tokens[i] = bytes(u2b[c] for c in t) if all(c in u2b for c in t) else t.encode('utf-8')
    merges = []
    with open(merges_txt, encoding='utf-8') as f:
        for n, line in enumerate(f.read().split('\n')):
            if (n == 0 and line.startswith('#version')) or not line.strip():
                continue
            parts = line.split(' ')
            if len(parts) != 2 or any(p not in vocab for p in parts + [''.join(parts)]):
                raise ValueError('{} line {}: {!r} is not two tokens whose join is one'.format(
                    merges_txt, n + 1, line))
            merges.append([vocab[parts[0]], vocab[parts[1]], vocab[parts[0] + parts[1]]])
    return tokens, vocab, np.asarray(merges, np.int32).reshape(-1, 3)


def load_tokenizer_json(path):
    """A Hugging Face tokenizer.json of a byte-level BPE -> (tokens, vocab, merges, options):
    load_tables' three, and BpeContext.from_tables' keywords pattern, ignore_merges and added
    (the added_tokens as content -> id; one outside model.vocab is a token without bytes, so
    no text reaches it). The pattern is known by its Split regex string, compared exactly."""
    if not isinstance(path, str) or not os.path.isfile(path):
        raise FileNotFoundError('tokenizer_json {!r}: a local file is required'.format(path))
    with open(path, encoding='utf-8') as f:
        try:
            js = json.load(f)
        except ValueError as e:
            raise ValueError('{}: not JSON ({})'.format(path, e)) from None
    model = js.get('model') if isinstance(js, dict) else None
    if not isinstance(model, dict) or model.get('type', 'BPE') != 'BPE' or \
            not isinstance(model.get('vocab'), dict) or not isinstance(model.get('merges'), list):
        raise ValueError('{}: no BPE model with vocab and merges'.format(path))
    pre = js.get('pre_tokenizer') or {}
    nodes = pre.get('pretokenizers', [pre]) if pre.get('type') == 'Sequence' else [pre]
    splits = [n for n in nodes if n.get('type') == 'Split']
    byte_level = [n for n in nodes if n.get('type') == 'ByteLevel']
    if len(byte_level) != 1 or byte_level[0].get('add_prefix_space') or len(splits) > 1:
        raise ValueError('{}: not a byte-level pre-tokenizer without a prefix space'.format(path))
    if splits:
        rx = splits[0].get('pattern', {}).get('Regex')
        if rx not in SPLIT_REGEX or byte_level[0].get('use_regex', True):
            raise ValueError('{}: unknown pre-tokenizer pattern {!r}'.format(path, rx))
        pattern = SPLIT_REGEX[rx]
    elif byte_level[0].get('use_regex', True):
        pattern = 'gpt2'
    else:
        raise ValueError('{}: the pre-tokenizer has no pattern'.format(path))
    vocab = dict(model['vocab'])
    if not vocab or not all(isinstance(k, str) and isinstance(v, int) and v >= 0 for k, v in vocab.items()) \
            or len(set(vocab.values())) != len(vocab):
        raise ValueError('{}: model.vocab is not an object of token -> distinct id'.format(path))
    added = {}
    for t in js.get('added_tokens') or []:
        if vocab.get(t['content'], t['id']) != t['id'] or (t['content'] not in vocab and
                                                           t['id'] in vocab.values()):
            raise ValueError('{}: added token {!r} clashes with model.vocab'.format(path, t['content']))
        added[t['content']] = t['id']
    u2b = {c: b for b, c in bytes_to_unicode().items()}
    tokens = [b''] * (max(list(vocab.values()) + list(added.values())) + 1)
    for t, i in vocab.items():
        tokens[i] = bytes(u2b[c] for c in t) if all(c in u2b for c in t) else t.encode('utf-8')
    merges = []
    for n, m in enumerate(model['merges']):
        parts = m.split(' ') if isinstance(m, str) else list(m)
        if len(parts) != 2 or any(p not in vocab for p in parts + [''.join(parts)]):
            raise ValueError('{} merge {}: {!r} is not two tokens whose join is one'.format(path, n, m))
        merges.append([vocab[parts[0]], vocab[parts[1]], vocab[parts[0] + parts[1]]])
    vocab.update(added)
    return tokens, vocab, np.asarray(merges, np.int32).reshape(-1, 3), dict(
        pattern=pattern, ignore_merges=bool(model.get('ignore_merges', False)), added=added)


def load_bpe_arg(bpe):
    """The loaders' bpe= -> (tokens, vocab, merges, BpeContext.from_tables' keywords): a
    tokenizer.json path, (vocab_json, merges_txt), or that pair followed by a dict of pattern,
    digit_group and ignore_merges."""
    if isinstance(bpe, str):
        return load_tokenizer_json(bpe)
    if not isinstance(bpe, (tuple, list)) or len(bpe) not in (2, 3) or \
            (len(bpe) == 3 and not isinstance(bpe[2], dict)):
        raise ValueError('bpe must be (vocab_json, merges_txt), that pair and a dict of keywords, '
                         'or a tokenizer.json path, not {!r}'.format(bpe))
    options = dict(bpe[2]) if len(bpe) == 3 else {}
    unknown = sorted(set(options) - {'pattern', 'digit_group', 'ignore_merges'})
    if unknown:
        raise ValueError('bpe keywords are pattern, digit_group and ignore_merges, not {}'.format(unknown))
    check_options(**options)
    return load_tables(*bpe[:2]) + (options,)


def load_classes(path=CLASSES):
    """The class table lddl_bpe_create takes (include/lddl_amd.h: header, l1, 64-byte pages of
    2-bit classes) from the ranges of assets/bpe_classes.txt (tools/bpe_classes.py) -> uint8
    array. The classes are the file's, not those of this interpreter's unicodedata."""
    with open(path) as f:
        lines = f.read().split('\n')
    version = [int(x) for x in lines[0].split('Unicode ')[1].split('.')]
    cls = np.zeros(0x110000, np.uint8)
    for ln in lines:
        if ln and not ln.startswith('#'):
            span, c = ln.split(' ')
            a, b = (int(x, 16) for x in span.split('..'))
            cls[a:b + 1] = ' LNS'.index(c)
    q = cls.reshape(-1, 64, 4)
    packed = (q[..., 0] | q[..., 1] << 2 | q[..., 2] << 4 | q[..., 3] << 6).astype(np.uint8)
    pages, l1 = np.unique(packed, axis=0, return_inverse=True)
    head = np.zeros(32, np.uint8)
    head[:4] = list(b'LBPC')
    head[4:8] = np.array([1], '<u4').view(np.uint8)
    head[8:11] = version
    head[12:20] = np.array([len(l1), len(pages)], '<u4').view(np.uint8)
    return np.concatenate([head, l1.reshape(-1).astype('<u2').view(np.uint8), pages.reshape(-1)])


def create_native(tokens, merges, device, classes=None):
    """lddl_bpe_create on byte strings and id triples -> handle (NativeError on a refusal)."""
    import ctypes
    from ._native import check, lib
    table = np.ascontiguousarray(load_classes() if classes is None else classes, np.uint8)
    off = np.zeros(len(tokens) + 1, np.int64)
    np.cumsum([len(t) for t in tokens], out=off[1:])
    blob = np.frombuffer(b''.join(tokens) + b'\0', np.uint8)
    m = np.ascontiguousarray(merges, np.int32).reshape(-1, 3)
    h = ctypes.c_void_p()
    check(lib.lddl_bpe_create(int(device), table.ctypes.data, len(table), blob.ctypes.data,
                              off.ctypes.data, len(tokens), m.ctypes.data, len(m), ctypes.byref(h)))
    return h


class BpeContext:
    """A byte-level BPE vocabulary resident in HBM; kernels run on torch's current stream."""

    def __init__(self, vocab_json, merges_txt, device=None, pattern='gpt2', digit_group=None,
                 ignore_merges=False):
        """pattern: 'gpt2' (GPT-2, RoBERTa, BART), 'cl100k' (Llama 3, GPT-4, DeepSeek; digits in
        groups of digit_group = 3) or 'qwen2' (cl100k with digit_group = 1). ignore_merges: a
        pre-token that is a vocabulary entry is that entry (Llama 3)."""
        options = check_options(pattern, digit_group, ignore_merges)
        self._attach(*load_tables(vocab_json, merges_txt), device, options)

    @classmethod
    def from_tables(cls, tokens, merges, device=None, vocab=None, pattern='gpt2', digit_group=None,
                    ignore_merges=False, added=None):
        """A context of tables already in memory (hand-built, or load_tables' with its vocab):
        tokens (bytes by id) and merges [n, 3] of (left, right, merged) ids in rank order, as
        lddl_bpe_create takes them. added: names -> ids that join special_ids."""
        options = check_options(pattern, digit_group, ignore_merges)
        self = cls.__new__(cls)
        if vocab is None:
            b2u = bytes_to_unicode()
            vocab = {''.join(b2u[b] for b in t): i for i, t in enumerate(tokens)}
        self._attach(list(tokens), vocab, np.asarray(merges, np.int32).reshape(-1, 3), device,
                     options, added)
        return self

    @classmethod
    def from_tokenizer_json(cls, path, device=None):
        """A context of a Hugging Face tokenizer.json (load_tokenizer_json)."""
        tokens, vocab, merges, options = load_tokenizer_json(path)
        return cls.from_tables(tokens, merges, device, vocab, **options)

    def _attach(self, tokens, vocab, merges, device, options=('gpt2', 0, False), added=None):
        self.tokens, self.vocab, self.merges = tokens, vocab, merges
        self.special_ids = {t: self.vocab.get(t, -1) for t in SPECIALS}
        self.special_ids.update(added or {})
        self.pattern, self.digit_group, self.ignore_merges = options
        import ctypes
        import torch
        from ._native import check, lib
        if not torch.cuda.is_available():
            raise RuntimeError('lddl_amd needs a ROCm GPU; there is no CPU fallback')
        self.device = torch.device('cuda', torch.cuda.current_device() if device is None else device)
        self._h = create_native(self.tokens, self.merges, self.device.index)
        if options != ('gpt2', 0, False):
            check(lib.lddl_bpe_set_pattern(self._h, self.pattern.encode(), self.digit_group))
            check(lib.lddl_bpe_set_whole_words(self._h, int(self.ignore_merges)))
        bits, n = ctypes.c_void_p(), ctypes.c_int64()
        check(lib.lddl_bpe_cont_bits(self._h, ctypes.byref(bits), ctypes.byref(n)))
        self.cont_bits = (bits, n.value)  # lddl_bart_denoise_bits' first two arguments
        self._b2u = bytes_to_unicode()

    @property
    def handle(self):
        return self._h

    def __len__(self):
        return len(self.tokens)

    def close(self):
        if getattr(self, '_h', None):
            from ._native import lib
            lib.lddl_bpe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def tokenize(self, text, sent_off, doc_sent_off=None, max_pieces=512):
        """text: uint8 cuda tensor; sent_off: int64 cuda tensor [n_sent + 1] from 0 to
        text.numel(); doc_sent_off: int64 cuda tensor [n_doc + 1] or None (every sentence a
        document). Returns (ids int32 [n_bytes], sent_len int32 [n_sent]) in ctx.tokenize's
        layout: sentence s's pieces are ids[sent_off[s] : sent_off[s] + sent_len[s]]."""
        import torch
        from ._native import check, lib
        from .context import _ptr, _stream
        assert text.dtype == torch.uint8 and text.is_cuda and text.is_contiguous()
        for t in (sent_off, doc_sent_off):
            assert t is None or (t.dtype == torch.int64 and t.is_cuda and t.is_contiguous())
        n_sent = sent_off.numel() - 1
        ids = torch.empty(max(text.numel(), 1), dtype=torch.int32, device=self.device)
        sent_len = torch.empty(max(n_sent, 0), dtype=torch.int32, device=self.device)
        check(lib.lddl_bpe_tokenize(
            self._h, _stream(), _ptr(text), text.numel(), _ptr(sent_off), n_sent,
            _ptr(doc_sent_off), 0 if doc_sent_off is None else doc_sent_off.numel() - 1,
            int(max_pieces), _ptr(ids), _ptr(sent_len)))
        return ids, sent_len

    def pretoken_stats(self, text, sent_off, doc_sent_off=None):
        """lddl_bpe_pretoken_stats on tokenize's input -> int64 cuda tensor [3]: pre-tokens,
        those of at most 64 bytes that cross their 64-byte tile's end, those over 64 bytes."""
        import torch
        from ._native import check, lib
        from .context import _ptr, _stream
        out = torch.empty(3, dtype=torch.int64, device=self.device)
        check(lib.lddl_bpe_pretoken_stats(
            self._h, _stream(), _ptr(text), text.numel(), _ptr(sent_off), sent_off.numel() - 1,
            _ptr(doc_sent_off), 0 if doc_sent_off is None else doc_sent_off.numel() - 1, _ptr(out)))
        return out

    def tokenize_host(self, text, sent_off, doc_sent_off=None, max_pieces=512):
        """Convenience: numpy in, ragged numpy (ids, offsets) out."""
        import torch
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(self.device)  # noqa: E731
        ids, sl = self.tokenize(dev(text, np.uint8), dev(sent_off, np.int64),
                                None if doc_sent_off is None else dev(doc_sent_off, np.int64),
                                max_pieces)
        ids, sl = ids.cpu().numpy(), sl.cpu().numpy().astype(np.int64)
        out_off = np.zeros(len(sl) + 1, np.int64)
        np.cumsum(sl, out=out_off[1:])
        so = np.asarray(sent_off, np.int64)
        flat = [ids[so[i]:so[i] + sl[i]] for i in range(len(sl))]
        return (np.concatenate(flat) if flat else np.zeros(0, np.int32)), out_off

    def encode(self, s):
        """The ids of one string (one sentence, one document), as GPT-2's encode."""
        b = np.frombuffer(s.encode('utf-8'), np.uint8)
        if not len(b):
            return []
        return self.tokenize_host(b, [0, len(b)], None, len(b))[0].tolist()

    def convert_ids_to_tokens(self, ids):
        """Ids -> the strings of vocab.json (GPT-2's byte-to-unicode form)."""
        one = lambda i: ''.join(self._b2u[b] for b in self.tokens[int(i)])  # noqa: E731
        return one(ids) if isinstance(ids, int) else [one(i) for i in ids]
