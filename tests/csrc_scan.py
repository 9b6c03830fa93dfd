'''
What the source scans of the per-library CPU tests read beside a library's one .hip: the shared headers under
danet-tensorflow_amd/csrc/ that the source includes (ext_core.h, ragged_rows.h, sumsq_f64.h, adam_one.h,
wave_metric.h).  A header of include/ is the library's ABI and is not source in this sense.
'''
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'danet-tensorflow_amd', 'csrc')


def strip_comments(text):
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def shared_headers(source_text):
    '''paths of the csrc/*.h the source text includes, in its order'''
    paths = [os.path.join(CSRC, h) for h in re.findall(r'#include "(\w+\.h)"', strip_comments(source_text))]
    return [p for p in paths if os.path.isfile(p)]


def shared_code(source_text, comments=False):
    '''the text of those headers one after the other, without /* */ comments unless they are asked for; a shared
    header includes no other, so this is all the library's own code outside its .hip'''
    texts = [open(p).read() for p in shared_headers(source_text)]
    assert texts and not any(shared_headers(t) for t in texts), source_text[:200]
    return '\n'.join(texts if comments else [strip_comments(t) for t in texts])
