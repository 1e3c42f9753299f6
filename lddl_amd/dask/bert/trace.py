"""LDDL_TRACE_PIPELINE=1: host timeline of the CLI pipeline on stderr (diagnostics)."""
import os
import sys
import time

_TRACE = os.environ.get('LDDL_TRACE_PIPELINE')


def trace(what, batch):
    if _TRACE:
        import threading
        sys.stderr.write('[pipe] %8.3f %-14s batch@%s %s\n' % (time.perf_counter(), what,
                                                               batch,
                                                               threading.current_thread().name))
