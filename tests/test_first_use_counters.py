"""The keypoint and refined-keypoint counters are allocated on first use and zeroed with hipMemset,
which runs on the null stream; a context's own stream is non-blocking and does not wait for it.
The zeroing must have landed before the first kernel on that stream counts into the buffer, else
it can land afterwards and wipe the count (seen once as "0 records, 3 expected" in the steady-state
sweep's refine event).  CPU: every first-use path (the context's two lists, and the orientation,
describe and match objects' counters and input-list sentinels) waits for the null stream.  GPU: the very first
detection and refinement of many fresh contexts count what a second run on the same context counts."""
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "sift-parallel-optimization_amd", "csrc")


def _function(src, head):
    """The text of the function whose definition starts with `head`, up to its closing brace."""
    body = src[src.index(head):]
    return body[:body.index("\n}")]


def test_first_use_zeroing_is_waited_for():
    with open(os.path.join(CSRC, "gdp.hip")) as f:
        src = f.read()
    # one function fills counters (zero, or the 0xff "no list" sentinel) and waits for the null stream after the fill
    fill = _function(src, "hipError_t alloc_counters(uint32_t** count, size_t n, int byte) {")
    m = re.search(r"hipMemset\(\*count, byte, [^;]*;(.*)", fill, re.S)
    assert m and "hipStreamSynchronize(nullptr)" in m.group(1)
    # ... and nothing else allocates a counter or fills one on the null stream
    rest = src.replace(fill, "")
    assert len(rest) < len(src)
    assert not re.search(r"\bhipMemset\([^;]*count", rest) and not re.search(r"\bhipMalloc\([^;]*count", rest)
    # a list's zeroed counters come from it, and both context lists are such lists on first use
    assert "alloc_counters(count, n, 0)" in _function(src, "hipError_t alloc_list(R** list, size_t records, uint32_t** count, size_t n) {")
    assert "alloc_list(list, c->kp_capacity * batch, count, batch)" in _function(src, "int ensure_list(gdp_ctx* c, R** list, ")
    for fn, args in (("ensure_keypoints", "&c->d_kp, &c->d_kp_count"), ("ensure_refined", "&c->d_rf, &c->d_rf_count")):
        assert f"int {fn}(gdp_ctx* c) {{ return ensure_list(c, {args}, " in src, fn
        assert src.count(args.split()[1]) == 1, fn  # the counter's address is taken nowhere else
    # the handle objects: the oriented, described and match counters and the d_in_count sentinels
    finish = _function(src, "int finish_create(W** out, W* w, ")
    assert "alloc_list(&w->d_out, w->capacity * batch, &w->d_count, batch)" in finish
    assert "alloc_counters(&w->d_in_count, batch, 0xff)" in finish
    for fn in ("gdp_orient_create", "gdp_describe_create"):
        assert "return finish_create(out, w, " in _function(src, f"int {fn}("), fn
    match = _function(src, "int gdp_match_create(")
    assert "alloc_list(&m->d_out, m->cap[0], &m->d_count, 1)" in match and "alloc_counters(&m->d_in_count, 2, 0xff)" in match


@pytest.mark.gpu
def test_first_detection_and_refinement_of_fresh_contexts_keep_their_counts(pkg, oracle):
    H, W, S = 64, 96, 2
    img = oracle.lcg_image(H, W, 4242)
    counts = set()
    for _ in range(24):
        with pkg.PyramidContext(H, W, S=S) as ctx:
            ctx.set_input(img)
            ctx.build()
            ctx.detect_extrema()
            ctx.refine_keypoints()  # the same stream, nothing in between: both buffers' first use
            first = (ctx.keypoint_count(0), ctx.refined_count(0))
            ctx.detect_extrema()
            ctx.refine_keypoints()
            assert first == (ctx.keypoint_count(0), ctx.refined_count(0))
            counts.add(first)
    assert len(counts) == 1 and min(counts.pop()) > 0
