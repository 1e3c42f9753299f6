"""Drop-in counterparts of lddl.torch (the reference's PyTorch loader package).

`get_bert_pretrain_data_loader`, `get_bert_pretrain_packed_data_loader` (sequence packing, past
the reference) and the online loaders (`get_bert_pretrain_online_data_loader`, `collate_pairs`:
raw text to batches without shards; `get_bert_pretrain_online_packed_data_loader`: the same with
sequence packing planned and collated on the device; both past the reference) and the compact
MLM targets (`compact_labels`, `CompactMLMTargets`: a `collate_fn` for every loader) are resolved
lazily, so that DataLoader workers started with `spawn` / `forkserver` import only the
worker-side modules (`packing`, `seqpack`, `datasets`), never the native library."""


def __getattr__(name):
    if name in ('get_bert_pretrain_data_loader', 'get_bert_pretrain_packed_data_loader'):
        from . import bert
        return getattr(bert, name)
    if name in ('get_bert_pretrain_online_data_loader', 'collate_pairs',
                'get_bert_pretrain_online_packed_data_loader', 'plan_rows_device',
                'collate_pairs_seqpacked'):
        from . import online
        return getattr(online, name)
    if name in ('compact_labels', 'CompactMLMTargets'):
        from . import targets
        return getattr(targets, name)
    raise AttributeError(name)
