"""SentencePiece unigram on the device: the tokenizer of T5, mT5, ALBERT, XLNet,
XLM-R and mBART checkpoints, from their `spiece.model`. `load_model` reads the file with a
protobuf wire reader of its own (no dependency on `sentencepiece` or `protobuf`),
`UnigramContext` hands byte strings, scores and types to lddl_unigram_create and wraps
lddl_unigram_tokenize (include/lddl_amd.h states the semantics). `load_normalizer` reads the
model's normalisation rules and byte pieces, which the context applies on the device (§33). Argument errors are raised
before the native library is imported.
"""
import os
import struct

import numpy as np

SPECIALS = ('</s>', '<pad>', '<unk>', '<s>', '<mask>')
MARK = b'\xe2\x96\x81'  # U+2581
MAX_WORD = 1024  # LDDL_UNIGRAM_MAX_WORD
MAX_NEST = 16    # LDDL_UNIGRAM_MAX_NEST
NORMAL, UNKNOWN, CONTROL, USER_DEFINED, UNUSED, BYTE = 1, 2, 3, 4, 5, 6


def _fields(buf):
    """(field number, wire type, value) of one protobuf message: an int for a varint, the bytes
    of a fixed32 / fixed64 / length-delimited field. ValueError on anything else."""
    i, n = 0, len(buf)

    def varint():
        nonlocal i
        v = shift = 0
        while True:
            if i >= n or shift > 63:
                raise ValueError('truncated varint')
            b = buf[i]
            i += 1
            v |= (b & 0x7F) << shift
            shift += 7
            if b < 0x80:
                return v

    while i < n:
        key = varint()
        wt = key & 7
        if wt == 0:
            val = varint()
        elif wt in (1, 2, 5):
            size = varint() if wt == 2 else (8 if wt == 1 else 4)
            if i + size > n:
                raise ValueError('truncated field')
            val = bytes(buf[i:i + size])
            i += size
        else:
            raise ValueError('wire type {}'.format(wt))
        yield key >> 3, wt, val


def load_model(path):
    """(pieces: list of bytes by id, scores float32, types int32, unk_id, ascii_ws) of a
    SentencePiece model file. FileNotFoundError, or ValueError on a file that is no unigram
    model with add_dummy_prefix, remove_extra_whitespaces and escape_whitespaces all true.
    ascii_ws (LDDL_UNIGRAM_ASCII_WS): the normaliser is not `identity`, so tab, LF, FF and CR
    are spaces as well. A USER_DEFINED piece gets the score SentencePiece encodes it with,
    characters * (the highest NORMAL score) - 0.1."""
    if not isinstance(path, str) or not os.path.isfile(path):
        raise FileNotFoundError('model_file {!r}: a local file is required'.format(path))
    with open(path, 'rb') as f:
        raw = f.read()
    pieces, scores, types = [], [], []
    name, ws = b'', {3: 1, 4: 1, 5: 1}
    try:
        for num, wt, val in _fields(raw):
            if num == 1 and wt == 2:
                p = {1: b'', 2: struct.pack('<f', 0.0), 3: NORMAL}
                p.update({k: v for k, _, v in _fields(val)})
                pieces.append(p[1])
                scores.append(struct.unpack('<f', p[2])[0])
                types.append(p[3])
            elif num == 2 and wt == 2:
                if dict((k, v) for k, _, v in _fields(val)).get(3, 1) != 1:
                    raise ValueError('model_type is not UNIGRAM')
            elif num == 3 and wt == 2:
                for k, _, v in _fields(val):
                    if k == 1:
                        name = v
                    elif k in ws:
                        ws[k] = v
    except (ValueError, struct.error, TypeError) as e:
        raise ValueError('{}: not a SentencePiece unigram model ({})'.format(path, e)) from None
    if not pieces or types.count(UNKNOWN) != 1:
        raise ValueError('{}: not a SentencePiece unigram model (no pieces, or not one '
                         'UNKNOWN piece)'.format(path))
    if not all(ws.values()):
        raise ValueError('{}: add_dummy_prefix, remove_extra_whitespaces and escape_whitespaces '
                         'must all be true'.format(path))
    scores, types = np.asarray(scores, np.float32), np.asarray(types, np.int32)
    if (types == NORMAL).any():
        top = float(scores[types == NORMAL].max())
        for i in np.flatnonzero(types == USER_DEFINED):
            scores[i] = len(pieces[i].decode('utf-8', 'replace')) * top - 0.1
    return pieces, scores, types, types.tolist().index(UNKNOWN), name != b'identity'


def _charsmap_rules(cm):
    """(keys, repls) of a precompiled_charsmap: a little-endian uint32 trie size, a Darts
    double-array of uint32 units, a blob of NUL-terminated replacements. The keys come from a
    bounds-checked walk of the array, breadth first, 255 labels of a level's nodes at a time."""
    if len(cm) < 4:
        raise ValueError('precompiled_charsmap: no trie size')
    size = struct.unpack('<I', cm[:4])[0]
    if size == 0 or size % 4 or 4 + size > len(cm):
        raise ValueError('precompiled_charsmap: a trie of {} bytes in {}'.format(size, len(cm) - 4))
    units = np.frombuffer(cm, '<u4', size // 4, 4).astype(np.int64)
    blob, n = cm[4 + size:], size // 4
    labels = np.arange(1, 256, dtype=np.int64)
    nodes, keys, found, depth = np.zeros(1, np.int64), [b''], [], 0
    while len(nodes):
        u = units[nodes]
        base = nodes ^ ((u >> 10) << ((u & 0x200) >> 6))
        if (base >= n).any():
            raise ValueError('precompiled_charsmap: a unit\'s offset leaves the array')
        for i in np.flatnonzero((u >> 8) & 1):
            if not keys[i]:
                raise ValueError('precompiled_charsmap: an empty key')
            found.append((keys[i], int(units[base[i]] & 0x7FFFFFFF)))
        nxt, nxt_keys = [], []
        for a in range(0, len(nodes), 4096):
            cand = base[a:a + 4096, None] ^ labels[None, :]
            ok = (cand < n) & ((units[np.minimum(cand, n - 1)] & 0x800000FF) == labels[None, :])
            r, c = np.nonzero(ok)
            nxt.append(cand[r, c])
            nxt_keys += [keys[a + i] + bytes((j + 1,)) for i, j in zip(r.tolist(), c.tolist())]
        nodes, keys = np.concatenate(nxt), nxt_keys
        depth += 1  # Darts shares suffixes, so paths outnumber units; a cycle shows as depth
        if depth > 256 or len(nodes) > 1 << 24:
            raise ValueError('precompiled_charsmap: the array is no trie')
    out_k, out_r = [], []
    for k, v in sorted(found):
        end = blob.find(b'\0', v) if v < len(blob) else -1
        if end < 0:
            raise ValueError('precompiled_charsmap: a value past the blob, or no terminator')
        out_k.append(k)
        out_r.append(blob[v:end])
    return out_k, out_r


def load_normalizer(path):
    """(keys, repls, byte_pieces) of a SentencePiece model file: the rules of
    normalizer_spec.precompiled_charsmap as two lists of bytes, sorted by key (an `identity`
    model, or one without a map, has none), and the ids of the BYTE pieces <0x00> .. <0xFF> as
    int32 [256], None unless all 256 are there. ValueError on a malformed map: an index that
    leaves the array or the blob, an empty key, a replacement without its terminator."""
    if not isinstance(path, str) or not os.path.isfile(path):
        raise FileNotFoundError('model_file {!r}: a local file is required'.format(path))
    with open(path, 'rb') as f:
        raw = f.read()
    cm, ids, i = b'', {}, 0
    try:
        for num, wt, val in _fields(raw):
            if num == 1 and wt == 2:
                p = {k: v for k, _, v in _fields(val)}
                name = p.get(1, b'')
                if p.get(3, NORMAL) == BYTE and len(name) == 6 and name[:3] == b'<0x' and name[5:] == b'>':
                    ids[int(name[3:5], 16)] = i
                i += 1
            elif num == 3 and wt == 2:
                for k, _, v in _fields(val):
                    if k == 2:
                        cm = v
    except (struct.error, TypeError) as e:
        raise ValueError('{}: not a SentencePiece model ({})'.format(path, e)) from None
    keys, repls = _charsmap_rules(cm) if cm else ([], [])
    return keys, repls, (np.array([ids[b] for b in range(256)], np.int32) if len(ids) == 256 else None)


def check_normalizer(normalizer, byte_pieces):
    """from_tables' normalizer=(keys, repls) and byte_pieces= as the native calls take them."""
    if normalizer is not None:
        keys, repls = ([k.encode('utf-8') if isinstance(k, str) else bytes(k) for k in x] for x in normalizer)
        if len(keys) != len(repls) or not keys:
            raise ValueError('normalizer: one replacement per key, one rule at least')
        normalizer = (keys, repls)
    if byte_pieces is not None:
        byte_pieces = np.ascontiguousarray(byte_pieces, np.int32).reshape(-1)
        if len(byte_pieces) != 256:
            raise ValueError('byte_pieces must be 256 ids')
    return normalizer, byte_pieces


def check_tables(pieces, scores, types=None, unk_id=0):
    """from_tables' arguments as create_native takes them (ValueError on mismatched shapes)."""
    pieces = [p.encode('utf-8') if isinstance(p, str) else bytes(p) for p in pieces]
    scores = np.ascontiguousarray(scores, np.float32).reshape(-1)
    if not isinstance(unk_id, int) or isinstance(unk_id, bool):
        raise ValueError('unk_id must be an int, not {!r}'.format(unk_id))
    if types is None:
        types = np.full(len(pieces), NORMAL, np.int32)
        if 0 <= unk_id < len(pieces):
            types[unk_id] = UNKNOWN
    types = np.ascontiguousarray(types, np.int32).reshape(-1)
    if not pieces or len(scores) != len(pieces) or len(types) != len(pieces):
        raise ValueError('pieces, scores and types must have one entry per piece, one at least')
    return pieces, scores, types, unk_id


def create_native(pieces, scores, types, unk_id, ascii_ws, device):
    """lddl_unigram_create on byte strings -> handle (NativeError on a refusal)."""
    import ctypes
    from ._native import check, lib
    off = np.zeros(len(pieces) + 1, np.int64)
    np.cumsum([len(p) for p in pieces], out=off[1:])
    blob = np.frombuffer(b''.join(pieces) + b'\0', np.uint8)
    h = ctypes.c_void_p()
    check(lib.lddl_unigram_create(int(device), blob.ctypes.data, off.ctypes.data, scores.ctypes.data,
                                  types.ctypes.data, len(pieces), int(unk_id), int(bool(ascii_ws)),
                                  ctypes.byref(h)))
    return h


class UnigramContext:
    """A unigram vocabulary resident in HBM; kernels run on torch's current stream."""

    def __init__(self, model_file, device=None):
        tables = load_model(model_file)
        keys, repls, byte_pieces = load_normalizer(model_file)
        self._attach(*tables, device, (keys, repls) if keys else None, byte_pieces)

    @classmethod
    def from_tables(cls, pieces, scores, types=None, unk_id=0, ascii_ws=False, device=None,
                    normalizer=None, byte_pieces=None):
        """A context of tables already in memory (hand-built, or load_model's): pieces (bytes or
        str by id), scores, types (None: all NORMAL but unk_id), as lddl_unigram_create takes
        them. normalizer=(keys, repls), two lists of bytes or str, and byte_pieces, 256 ids, are
        load_normalizer's; with both None the context is that of §32."""
        self = cls.__new__(cls)
        tables = check_tables(pieces, scores, types, unk_id)
        self._attach(*tables, bool(ascii_ws), device, *check_normalizer(normalizer, byte_pieces))
        return self

    def _attach(self, pieces, scores, types, unk_id, ascii_ws, device, normalizer=None, byte_pieces=None):
        self.pieces, self.scores, self.types = pieces, scores, types
        self.unk_id, self.ascii_ws = unk_id, ascii_ws
        names = {p: i for i, p in reversed(list(enumerate(pieces)))}
        self.special_ids = {t: names.get(t.encode(), -1) for t in SPECIALS}
        import ctypes
        import torch
        from ._native import check, lib
        if not torch.cuda.is_available():
            raise RuntimeError('lddl_amd needs a ROCm GPU; there is no CPU fallback')
        self.device = torch.device('cuda', torch.cuda.current_device() if device is None else device)
        self._h = create_native(pieces, scores, types, unk_id, ascii_ws, self.device.index)
        bits, n = ctypes.c_void_p(), ctypes.c_int64()
        check(lib.lddl_unigram_cont_bits(self._h, ctypes.byref(bits), ctypes.byref(n)))
        self.cont_bits = (bits, n.value)  # lddl_bart_denoise_bits' first two arguments
        self.rules = 0
        if normalizer is not None:
            blobs = []
            for strings in normalizer:
                off = np.zeros(len(strings) + 1, np.int64)
                np.cumsum([len(x) for x in strings], out=off[1:])
                blobs += [np.frombuffer(b''.join(strings) + b'\0', np.uint8), off]
            check(lib.lddl_unigram_set_normalizer(self._h, *(a.ctypes.data for a in blobs), len(normalizer[0])))
            self.rules = len(normalizer[0])
        if byte_pieces is not None:
            check(lib.lddl_unigram_set_byte_pieces(self._h, byte_pieces.ctypes.data))

    @property
    def handle(self):
        return self._h

    def __len__(self):
        return len(self.pieces)

    def close(self):
        if getattr(self, '_h', None):
            from ._native import lib
            lib.lddl_unigram_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """lddl_unigram_info and lddl_unigram_norm_info -> dict of pieces, nodes, table_bytes,
        unk_score, max_word; rules, max_key, max_repl (bytes), byte_fallback."""
        import ctypes
        from ._native import check, lib
        a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        u, w = ctypes.c_float(), ctypes.c_int32()
        check(lib.lddl_unigram_info(self._h, *(ctypes.addressof(v) for v in (a, b, c, u, w))))
        r, k, m, f = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        check(lib.lddl_unigram_norm_info(self._h, *(ctypes.addressof(v) for v in (r, k, m, f))))
        return {'pieces': a.value, 'nodes': b.value, 'table_bytes': c.value, 'unk_score': u.value,
                'max_word': w.value, 'rules': r.value, 'max_key': k.value, 'max_repl': m.value,
                'byte_fallback': bool(f.value)}

    def continuation_ids(self):
        """The ids whose bit is set in the continuation bitmap (lddl_unigram_cont_bits): the
        pieces that never begin a word."""
        from ._native import check, lib
        bits = np.zeros((len(self.pieces) + 31) // 32, np.uint32)
        check(lib.lddl_unigram_cont_bits_host(self._h, bits.ctypes.data))
        return [i for i in range(len(self.pieces)) if bits[i >> 5] >> np.uint32(i & 31) & 1]

    def normalize(self, text, sent_off, out_cap=None):
        """The model's normaliser on tokenize's input -> (text2, sent_off2), the
        input itself if no normaliser is set. lddl_unigram_normalize_plan, one read-back of the
        planned size (the one host wait: the output is allocated by it), then
        lddl_unigram_normalize_write. out_cap: the capacity handed to the write instead of the
        planned size (NativeError if it is too small)."""
        import torch
        from ._native import check, lib
        from .context import _ptr, _stream
        if not self.rules:
            return text, sent_off
        assert text.dtype == torch.uint8 and text.is_cuda and text.is_contiguous()
        assert sent_off.dtype == torch.int64 and sent_off.is_cuda and sent_off.is_contiguous()
        n_sent = sent_off.numel() - 1
        so2 = torch.empty(n_sent + 1, dtype=torch.int64, device=self.device)
        head = (self._h, _stream(), _ptr(text), text.numel(), _ptr(sent_off), n_sent, _ptr(so2))
        check(lib.lddl_unigram_normalize_plan(*head))
        size = int(so2[-1].item())
        cap = size if out_cap is None else int(out_cap)
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=self.device)
        check(lib.lddl_unigram_normalize_write(*head, _ptr(out), cap))
        return out[:size], so2

    def _call(self, fn, text, sent_off, doc_sent_off, *tail):
        import torch
        from ._native import check
        from .context import _ptr, _stream
        assert text.dtype == torch.uint8 and text.is_cuda and text.is_contiguous()
        for t in (sent_off, doc_sent_off):
            assert t is None or (t.dtype == torch.int64 and t.is_cuda and t.is_contiguous())
        check(fn(self._h, _stream(), _ptr(text), text.numel(), _ptr(sent_off), sent_off.numel() - 1,
                 _ptr(doc_sent_off), 0 if doc_sent_off is None else doc_sent_off.numel() - 1,
                 *tail))

    def tokenize(self, text, sent_off, doc_sent_off=None, max_pieces=512):
        """text: uint8 cuda tensor; sent_off: int64 cuda tensor [n_sent + 1] from 0 to
        text.numel(); doc_sent_off: accepted for BpeContext.tokenize's signature, unread.
        Returns (ids int32 [n_bytes], sent_len int32 [n_sent]) in ctx.tokenize's layout:
        sentence s's pieces are ids[sent_off[s] : sent_off[s] + sent_len[s]]."""
        import torch
        from ._native import lib
        from .context import _ptr
        n_sent = sent_off.numel() - 1
        ids = torch.empty(max(text.numel(), 1), dtype=torch.int32, device=self.device)
        sent_len = torch.empty(max(n_sent, 0), dtype=torch.int32, device=self.device)
        self._call(lib.lddl_unigram_tokenize, text, sent_off, doc_sent_off, int(max_pieces),
                   _ptr(ids), _ptr(sent_len))
        return ids, sent_len

    def word_stats(self, text, sent_off, doc_sent_off=None):
        """lddl_unigram_word_stats on tokenize's input -> int64 cuda tensor [3]: words, those of
        at most 64 bytes that cross their 64-byte tile's end, those over 64 bytes."""
        import torch
        from ._native import lib
        from .context import _ptr
        out = torch.empty(3, dtype=torch.int64, device=self.device)
        self._call(lib.lddl_unigram_word_stats, text, sent_off, doc_sent_off, _ptr(out))
        return out

    def tokenize_host(self, text, sent_off, doc_sent_off=None, max_pieces=512):
        """Convenience: numpy in, ragged numpy (ids, offsets) out; normalised first if a
        normaliser is set."""
        import torch
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(self.device)  # noqa: E731
        text, so = self.normalize(dev(text, np.uint8), dev(sent_off, np.int64))
        ids, sl = self.tokenize(text, so, None if doc_sent_off is None else dev(doc_sent_off, np.int64),
                                max_pieces)
        ids, sl = ids.cpu().numpy(), sl.cpu().numpy().astype(np.int64)
        out_off = np.zeros(len(sl) + 1, np.int64)
        np.cumsum(sl, out=out_off[1:])
        so = so.cpu().numpy()
        flat = [ids[so[i]:so[i] + sl[i]] for i in range(len(sl))]
        return (np.concatenate(flat) if flat else np.zeros(0, np.int32)), out_off

    def encode(self, s):
        """The ids of one string (one sentence), as SentencePiece's EncodeAsIds up to the stated
        deviations. A sentence of words without their own mark pieces can have more pieces than
        bytes; the layout keeps the first `bytes` of them."""
        b = np.frombuffer(s.encode('utf-8'), np.uint8)
        if not len(b):
            return []
        return self.tokenize_host(b, [0, len(b)], None, 1 << 30)[0].tolist()

    def convert_ids_to_tokens(self, ids):
        """Ids -> the piece strings of the model."""
        one = lambda i: self.pieces[int(i)].decode('utf-8', 'replace')  # noqa: E731
        return one(ids) if isinstance(ids, int) else [one(i) for i in ids]
