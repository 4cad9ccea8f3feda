"""The stream case table (tests/stream_cases.py) against the C ABI (include/gdx.h), no GPU needed: every function that takes a
`stream` has a case in tests/test_gpu_streams.py or a written reason why not, and the table names nothing the header lacks."""
import os
import re

import stream_cases as SC
from conftest import REPO
from gesturediffusion_amd._lib import parse_header

HDR = open(os.path.join(REPO, "include", "gdx.h")).read()


def stream_entries(text):
    """The functions of a header that take a parameter named `stream`, in declaration order."""
    return [name for name, (_, params) in parse_header(text).prototypes.items() if any(p == "stream" for _, p in params)]


def missing_and_stale(text):
    takes = set(stream_entries(text))
    known = set(SC.ENTRY_CASES) | set(SC.EXEMPT)
    return sorted(takes - known), sorted(known - takes)


def test_every_stream_taking_entry_has_a_case_or_a_reason():
    entries = stream_entries(HDR)
    # the parser's count against a plain search of the comment-free text: a declaration it skipped would hide an entry
    bare = re.sub(r"/\*.*?\*/|//[^\n]*", " ", HDR, flags=re.S)
    assert len(entries) == len(re.findall(r"void\s*\*\s*stream\s*\)\s*;", bare)) > 50
    missing, stale = missing_and_stale(HDR)
    assert not missing, f"entries of gdx.h that take a stream and have neither a case nor a reason in tests/stream_cases.py: {missing}"
    assert not stale, f"tests/stream_cases.py names entries that gdx.h does not declare with a stream parameter: {stale}"
    assert not set(SC.ENTRY_CASES) & set(SC.EXEMPT)


def test_a_new_stream_taking_declaration_fails_until_it_has_a_case():
    """The check above on a header with one more entry, and on one with an entry less."""
    more = HDR.replace("int gdx_prepare(", "int gdx_new_kernel(const float* x, float* out, void* stream);\nint gdx_prepare(")
    assert more != HDR and missing_and_stale(more) == (["gdx_new_kernel"], [])
    less = re.sub(r"int gdx_randn\(.*?\);", "", HDR, flags=re.S)
    assert less != HDR and missing_and_stale(less) == ([], ["gdx_randn"])
    # a stream parameter that is dropped from a declaration makes its name stale too
    dropped = HDR.replace("int64_t count, void* stream);", "int64_t count);")
    assert dropped != HDR and missing_and_stale(dropped) == ([], ["gdx_get_tap"])


def test_table_is_well_formed():
    for name, e in SC.ENTRY_CASES.items():
        assert e["cases"] and isinstance(e["syncs"], bool), name
        assert len(set(e["cases"])) == len(e["cases"]), name
    for name, why in SC.EXEMPT.items():
        assert len(why) > 40 and ("alias" in why or "timing hook" in why), name
    assert len(set(SC.PROTOCOL_CASES)) == len(SC.PROTOCOL_CASES) and set(SC.SYNCS) == set(SC.PROTOCOL_CASES)
    # the entries whose own code synchronises the stream, as the header says of them
    for name in ("gdx_export_packed", "gdx_import_packed", "gdx_check_guards", "gdx_parallel_loop"):
        assert SC.ENTRY_CASES[name]["syncs"], name
    for name, e in SC.ENTRY_CASES.items():
        if name in SC.TEST_ENTRIES:
            assert e["syncs"], name
    for name in ("gdx_forward", "gdx_sample_loop", "gdx_set_condition", "gdx_sampler_update", "gdx_mfcc", "gdx_bpd_loop"):
        assert not SC.ENTRY_CASES[name]["syncs"], name
    # every forward shape in every mode, the 16-bit modes where the shape has them
    assert len(SC.FORWARD) == 3 * (5 * 3 + 1) and len(SC.SPECIAL) == 5
