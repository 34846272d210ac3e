"""The stream contract table (tests/stream_cases.py) against the public header and against the GPU test module: no _dev
entry without a row, no stale row, every row's kind in the header's own words, every row run by a GPU test that exists.
Needs no GPU and does not load the library."""
import ast
import os
import re

import stream_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "zkt_plonk.h")


def _declared():
    """declared_symbols() of zkt_plonk_amd._lib, restated so that the package (numpy, the library path) is not needed."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zkt_[a-z0-9_]+)\s*\(", text)))


def _plain(comment):
    """A block comment's words on one line."""
    body = comment[2:-2]
    return " ".join(re.sub(r"^\s*\*\s?", "", line).strip() for line in body.splitlines()).strip()


def _comments():
    """[(start, end, words)] of the block comments that begin a line, in order."""
    text = open(HEADER).read()
    return text, [(m.start(), m.end(), _plain(m.group(0))) for m in re.finditer(r"^/\*.*?\*/", text, flags=re.S | re.M)]


def _governing(symbol):
    """The words of the comment in front of the declaration of `symbol` (the nearest one that begins a line)."""
    text, comments = _comments()
    stripped = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)      # same offsets, comments blanked
    m = re.search(r"\b%s\s*\(" % re.escape(symbol), stripped)
    assert m, "%s is not declared in the header" % symbol
    before = [c for c in comments if c[1] <= m.start()]
    assert before, symbol
    return before[-1][2]


def _conventions():
    return _comments()[1][0][2]


def test_the_declared_symbols_are_read_as_the_package_reads_them():
    from zkt_plonk_amd import _lib
    assert _declared() == _lib.declared_symbols()


def test_every_dev_entry_has_a_row_and_no_row_is_stale():
    declared = _declared()
    dev = [s for s in declared if s.endswith("_dev")]
    assert len(dev) >= 19                                    # the parse found them
    rows = {r.symbol for r in SC.ROWS}
    missing = [s for s in dev + list(SC.REQUIRED) if s not in rows]
    assert not missing, "entries without a row in tests/stream_cases.py (and so without a stream test): %s" % missing
    stale = sorted(rows - set(declared))
    assert not stale, "rows for entries the header no longer declares: %s" % stale
    other = sorted(s for s in rows if not s.endswith("_dev") and s not in SC.REQUIRED)
    assert not other, "rows outside the table's scope: %s" % other


def test_the_kind_of_every_row_is_what_the_header_says():
    conventions = _conventions()
    assert "_dev suffix" in conventions
    for r in SC.ROWS:
        assert r.kind in (SC.ENQUEUE_ONLY, SC.SYNCHRONISES), r.symbol
        if r.exempt:
            continue
        own = _governing(r.symbol)
        where = own if r.where == SC.OWN else conventions
        assert r.words in where, "%s: the header does not say %r %s" % (
            r.symbol, r.words, "in front of the declaration" if r.where == SC.OWN else "in its conventions")
        other = SC.SYNCHRONISES if r.kind == SC.ENQUEUE_ONLY else SC.ENQUEUE_ONLY
        assert any(re.search(p, r.words) for p in SC.WORDS_OF[r.kind]), "%s: %r does not say %s" % (r.symbol, r.words, r.kind)
        assert not any(re.search(p, r.words) for p in SC.WORDS_OF[other]), "%s: %r says %s" % (r.symbol, r.words, other)
        if r.where == SC.CONVENTIONS:                        # the general rule holds only where the entry's own comment is silent
            said = [p for kind in SC.WORDS_OF.values() for p in kind if re.search(p, own)]
            assert not said, "%s: its own comment speaks (%s); quote that instead of the conventions" % (r.symbol, said)


def test_rows_are_complete():
    for r in SC.ROWS:
        assert isinstance(r.reads, list) and isinstance(r.writes, list), r.symbol
        if r.exempt:
            assert r.symbol.startswith("zkt_debug_"), "%s: only zkt_debug_* entries may be exempt" % r.symbol
            assert len(r.exempt.split()) >= 8 and r.test is None, "%s: an exemption needs its reason written out" % r.symbol
        else:
            assert r.form and r.wrapper and r.test, r.symbol
            assert r.reads or r.writes or r.kind == SC.SYNCHRONISES, r.symbol


def test_every_row_names_a_gpu_test_that_calls_it():
    path = os.path.join(HERE, SC.GPU_MODULE + ".py")
    src = open(path).read()
    tree = ast.parse(src)
    assert any(isinstance(n, ast.Assign) and any(getattr(t, "id", "") == "pytestmark" for t in n.targets) and "gpu" in ast.get_source_segment(src, n)
               for n in tree.body), "the module is not marked gpu"
    funcs = {n.name: ast.get_source_segment(src, n) for n in tree.body if isinstance(n, ast.FunctionDef)}

    def reaches(name, wrapper, seen):
        """the test, or a module-level helper it calls, calls ctx.<wrapper>"""
        body = funcs[name]
        if re.search(r"\.%s\b" % re.escape(wrapper), body):
            return True
        seen.add(name)
        return any(reaches(h, wrapper, seen) for h in funcs if h not in seen and re.search(r"\b%s\(" % re.escape(h), body))

    for r in SC.ROWS:
        if r.exempt:
            continue
        assert r.test in funcs and r.test.startswith("test_"), "%s: no test %s in %s" % (r.symbol, r.test, SC.GPU_MODULE)
        assert reaches(r.test, r.wrapper, set()), "%s: %s never calls Context.%s" % (r.symbol, r.test, r.wrapper)
    from zkt_plonk_amd import _lib
    for r in SC.ROWS:
        if not r.exempt:
            assert callable(getattr(_lib.Context, r.wrapper)), r.wrapper
            # the wrapper is the one that calls the row's symbol
            import inspect
            text = inspect.getsource(_lib.Context)
            assert r.symbol in text, r.symbol
