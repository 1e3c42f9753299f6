"""Drop-in counterparts of lddl.torch_mp (the reference's loader for tensor- / pipeline-parallel
training): samples follow the data-parallel rank, so every rank of one model-parallel group
yields the same batches, and static-masking batches carry the [B, L] loss mask.

Everything but the entry points is lddl_amd.torch's code, parameterised by `dp_rank`.
`get_bert_pretrain_data_loader` is resolved lazily, as in lddl_amd.torch: DataLoader workers
import only the worker-side modules, never the native library."""


def __getattr__(name):
    if name == 'get_bert_pretrain_data_loader':
        from .bert import get_bert_pretrain_data_loader
        return get_bert_pretrain_data_loader
    raise AttributeError(name)
