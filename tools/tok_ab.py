"""Tokenizer A/B (diagnostic): time lddl_tokenize over one synthetic batch with each
LDDL_TOKENIZE_PATH value and library given, and check every variant's ids / sent_len bit for bit
against the first one's.

    python tools/tok_ab.py <bytes> <variant>...   variant = [path][@lib-dir], e.g. batch  plain
    batch@lddl_amd/_lib_x  (path '' or batch = the default kernel)

Every variant runs in a child process of its own (a process loads one library), one after the
other; a child prints its time and the SHA-256 of sent_len and of every sentence's kept pieces,
and the digests are compared here. Other knobs (LDDL_TOKENIZE_SLOW, ...) pass through the
environment to all variants.
"""
import hashlib
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(nbytes, path):
    import torch
    sys.path.insert(0, REPO)
    from lddl_amd import synth
    from lddl_amd.context import Context
    corp = synth.generate(seed=1234, n_bytes=nbytes, nonascii_frac=0.01, threads=16)
    ctx = Context(os.path.join(REPO, 'lddl_amd', 'assets', 'vocab_synth_uncased_30522.txt'))
    text = torch.from_numpy(corp.text).cuda()
    off = torch.from_numpy(corp.sent_off).cuda()
    if path in ('', 'batch'):
        os.environ.pop('LDDL_TOKENIZE_PATH', None)
    else:
        os.environ['LDDL_TOKENIZE_PATH'] = path
    for _ in range(2):
        ids, sl = ctx.tokenize(text, off)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 5
    e0.record()
    for _ in range(n):
        ids, sl = ctx.tokenize(text, off)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    # the sparse ids layout: hash only each sentence's kept pieces
    h = hashlib.sha256(sl.cpu().numpy().tobytes())
    L = (sl & ((1 << 30) - 1)).to(torch.int64)
    so = off[:-1]
    k = torch.arange(int(L.max()), device=L.device)
    for c0 in range(0, len(L), 1 << 20):
        Lc, sc = L[c0:c0 + (1 << 20)], so[c0:c0 + (1 << 20)]
        m = k[None, :] < Lc[:, None]
        h.update(ids[(sc[:, None] + k[None, :])[m]].cpu().numpy().tobytes())
    print(json.dumps({'ms': ms, 'pieces': int(L.sum()), 'digest': h.hexdigest()}), flush=True)


def main():
    nbytes = int(float(sys.argv[1]))
    if len(sys.argv) > 3 and sys.argv[2] == '--child':
        return child(nbytes, sys.argv[3])
    ref = None
    for v in sys.argv[2:] or ['batch']:
        path, _, libdir = v.partition('@')
        env = dict(os.environ)
        if libdir:
            env['LDDL_AMD_LIB'] = os.path.join(os.path.abspath(libdir), 'liblddl_amd.so')
        r = subprocess.run([sys.executable, os.path.abspath(__file__), sys.argv[1], '--child', path or 'batch'],
                           env=env, stdout=subprocess.PIPE, text=True, timeout=900)
        if r.returncode != 0:
            sys.exit('[{}] failed with exit status {}'.format(v, r.returncode))
        res = json.loads(r.stdout.strip().splitlines()[-1])
        same = None if ref is None else res['digest'] == ref
        if ref is None:
            ref = res['digest']
        print('[{}] {:.3f} ms per {:.2f} GB, {:.2f} GB/s text, pieces {} bit-exact vs first: {}'.format(
            v, res['ms'], nbytes / 1e9, nbytes / res['ms'] / 1e6, res['pieces'], same), flush=True)


if __name__ == '__main__':
    main()
