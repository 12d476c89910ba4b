"""Nothing slips out of the hipGraph replay table (tests/test_graph_replay_gpu.py): every function include/apa.h
declares with a `stream` parameter is named by a row of ROWS, by NOT_CAPTURED (with its reason, and with a sentence in
the header that takes it out of the capturability claim) or by CAPTURED_ELSEWHERE (an existing test that captures it).
No device is touched: the table is plain data."""
import os
import re

from tests import test_graph_replay_gpu as table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'apa.h')


def stream_taking(text):
    """names of the declared apa_* functions whose parameter list contains `stream`, in header order"""
    code = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    code = re.sub(r'//[^\n]*', ' ', code)
    decls = re.findall(r'\b(apa_\w+)\s*\(([^;{}()]*)\)\s*;', code)
    return [name for name, params in decls if re.search(r'\bstream\b', params)]


def _header():
    with open(HEADER) as f:
        return f.read()


def covered(rows):
    return {e for r in rows for e in r['entries']}


def missing(text, rows, not_captured, elsewhere):
    have = covered(rows) | set(not_captured) | set(elsewhere)
    return [n for n in stream_taking(text) if n not in have]


def test_the_parser_finds_the_stream_taking_declarations():
    names = stream_taking(_header())
    assert len(names) == len(set(names)) == 70, len(names)
    for n in ('apa_attn_pool_fwd', 'apa_attn_head_train_epoch_cached', 'apa_pose_attn_train_step', 'apa_prof_event_record',
              'apa_clip_by_norm_prepare', 'apa_epoch_order', 'apa_preprocess_images'):
        assert n in names, n
    for n in ('apa_version', 'apa_pose_to_heatmap', 'apa_attn_pool_workspace_bytes', 'apa_image_aug_size',
              'apa_prof_event_create'):
        assert n not in names, n
    # a struct member or a comment that says `stream` declares nothing
    assert stream_taking('/* int apa_x(void* stream); */ typedef struct s { void* stream; } s; int apa_y(int a);') == []
    assert stream_taking('int apa_new_thing(const float* x,\n   int n, void* stream);') == ['apa_new_thing']


def test_every_stream_taking_entry_point_has_a_row_or_a_reason():
    assert missing(_header(), table.ROWS, table.NOT_CAPTURED, table.CAPTURED_ELSEWHERE) == []


def test_the_table_names_only_what_the_header_declares():
    names = set(stream_taking(_header()))
    for r in table.ROWS:
        assert r['entries'] and set(r['entries']) <= names, r['id']
        assert r['rule'] == table.BITS and callable(getattr(table, '_b_' + r['build'])), r['id']
    ids = [r['id'] for r in table.ROWS]
    assert len(ids) == len(set(ids))
    assert set(table.NOT_CAPTURED) <= names and set(table.CAPTURED_ELSEWHERE) <= names
    assert not covered(table.ROWS) & set(table.NOT_CAPTURED)
    for name, reason in table.NOT_CAPTURED.items():
        assert len(reason) > 20, name
    for name, where in table.CAPTURED_ELSEWHERE.items():
        path, test = where.split('::')
        with open(os.path.join(ROOT, path)) as f:
            src = f.read()
        assert 'def %s(' % test in src and 'torch.cuda.graph(' in src, where


def test_a_deleted_row_or_a_new_declaration_fails_with_the_name():
    text = _header()
    rows = [r for r in table.ROWS if 'apa_epoch_order' not in r['entries']]
    assert missing(text, rows, table.NOT_CAPTURED, table.CAPTURED_ELSEWHERE) == ['apa_epoch_order']
    grown = text.replace('#ifdef __cplusplus\n}', 'int apa_brand_new_op(float* x, void* stream);\n#ifdef __cplusplus\n}')
    assert grown != text
    assert missing(grown, table.ROWS, table.NOT_CAPTURED, table.CAPTURED_ELSEWHERE) == ['apa_brand_new_op']


def test_the_header_names_what_it_no_longer_covers():
    """the capturability sentence of include/apa.h excepts exactly the entries of NOT_CAPTURED, by name"""
    text = _header()
    m = re.search(r'hipGraph-capturable.*?exceptions(.*?)A capture freezes', text, flags=re.S)
    assert m, 'the conventions paragraph of include/apa.h changed its shape'
    excepted = set(re.findall(r'apa_\w+', m.group(1)))
    assert excepted == set(table.NOT_CAPTURED), (sorted(excepted), sorted(table.NOT_CAPTURED))
