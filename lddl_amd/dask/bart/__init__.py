"""Drop-in counterpart of `lddl.dask.bart` (the reference's BART pretraining preprocessor)."""
