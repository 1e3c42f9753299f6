"""Drop-in counterparts of lddl.torch (the reference's PyTorch loader package).

`get_bert_pretrain_data_loader`, `get_bert_pretrain_packed_data_loader` (sequence packing, past
the reference) and the online loader (`get_bert_pretrain_online_data_loader`, `collate_pairs`:
raw text to batches without shards, past the reference) are resolved lazily, so that DataLoader
workers started with `spawn` / `forkserver` import only the worker-side modules (`packing`,
`seqpack`, `datasets`), never the native library."""


def __getattr__(name):
    if name in ('get_bert_pretrain_data_loader', 'get_bert_pretrain_packed_data_loader'):
        from . import bert
        return getattr(bert, name)
    if name in ('get_bert_pretrain_online_data_loader', 'collate_pairs'):
        from . import online
        return getattr(online, name)
    raise AttributeError(name)
