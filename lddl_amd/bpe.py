"""Byte-level BPE on the device: GPT-2's tokenizer, which RoBERTa and BART
checkpoints share, from `vocab.json` and `merges.txt`. `BpeContext` undoes JSON and GPT-2's
byte-to-unicode map, hands raw byte strings and (left, right, merged) id triples in rank order
to lddl_bpe_create, and wraps lddl_bpe_tokenize (include/lddl_amd.h states the semantics).
Argument errors are raised before the native library is imported.
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

    def __init__(self, vocab_json, merges_txt, device=None):
        self._attach(*load_tables(vocab_json, merges_txt), device)

    @classmethod
    def from_tables(cls, tokens, merges, device=None, vocab=None):
        """A context of tables already in memory (hand-built, or load_tables' with its vocab):
        tokens (bytes by id) and merges [n, 3] of (left, right, merged) ids in rank order, as
        lddl_bpe_create takes them."""
        self = cls.__new__(cls)
        if vocab is None:
            b2u = bytes_to_unicode()
            vocab = {''.join(b2u[b] for b in t): i for i, t in enumerate(tokens)}
        self._attach(list(tokens), vocab, np.asarray(merges, np.int32).reshape(-1, 3), device)
        return self

    def _attach(self, tokens, vocab, merges, device):
        self.tokens, self.vocab, self.merges = tokens, vocab, merges
        self.special_ids = {t: self.vocab.get(t, -1) for t in SPECIALS}
        import ctypes
        import torch
        from ._native import check, lib
        if not torch.cuda.is_available():
            raise RuntimeError('lddl_amd needs a ROCm GPU; there is no CPU fallback')
        self.device = torch.device('cuda', torch.cuda.current_device() if device is None else device)
        self._h = create_native(self.tokens, self.merges, self.device.index)
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
