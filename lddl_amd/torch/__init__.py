"""Drop-in counterparts of lddl.torch (the reference's PyTorch loader package).

`get_bert_pretrain_data_loader`, `get_bert_pretrain_packed_data_loader` (sequence packing, past
the reference) and the online loaders (`get_bert_pretrain_online_data_loader`, `collate_pairs`:
raw text to batches without shards; `get_bert_pretrain_online_packed_data_loader`: the same with
sequence packing planned and collated on the device; both past the reference) and the compact
MLM targets (`compact_labels`, `CompactMLMTargets`: a `collate_fn` for every loader) and BART
denoising (`bart_denoise`, `get_bart_pretrain_data_loader`; past the reference) and the RoBERTa
loader (`roberta_blocks`, `collate_blocks`, `get_roberta_pretrain_data_loader`: FULL- and
DOC-SENTENCES blocks cut and collated on the device; past the reference) and T5 span corruption
(`t5_corrupt`, `t5_lengths`, `t5_tokens_length`, `get_t5_pretrain_data_loader`: exact-count
spans and sentinel rows from the same blocks; past the reference) and the GPT loader
(`stream_plan`, `collate_stream`, `get_gpt_pretrain_data_loader`: documents packed across rows
for causal language modelling, with optional fill-in-the-middle; past the reference) are resolved lazily, so that DataLoader workers started with `spawn` / `forkserver` import only the
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
    if name in ('bart_denoise', 'get_bart_pretrain_data_loader'):
        from . import denoise
        return getattr(denoise, name)
    if name in ('roberta_blocks', 'collate_blocks', 'get_roberta_pretrain_data_loader'):
        from . import roberta
        return getattr(roberta, name)
    if name in ('t5_lengths', 't5_tokens_length', 't5_corrupt', 'get_t5_pretrain_data_loader'):
        from . import t5
        return getattr(t5, name)
    if name in ('stream_plan', 'collate_stream', 'get_gpt_pretrain_data_loader'):
        from . import gpt
        return getattr(gpt, name)
    raise AttributeError(name)
