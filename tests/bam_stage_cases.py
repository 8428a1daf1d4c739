"""What tests/test_bam_stage.py and tests/test_bam_stage_gpu.py share (test support, not a test): the runs of sort_bam, markdup_bam and
index_bam whose complete output files are held against recorded SHA-256 digests (tests/golden/bam_stage_digests.json), and the program that
records them:

    python tests/bam_stage_cases.py          # host backend, --bgzf_deflate host; rewrites the JSON

The recorded bytes are those of the host backend with the project's own compressor (hostsrc/host_deflate.cpp), which depend on the tree
alone; zlib's blocks are not recorded, they depend on the zlib build.  The device writes the twin's bytes, so the same digests hold for
backend="device", deflate="device".  The counts are the result dicts without the input's size, the backend's name and the path."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import index_bam_cases as ic  # noqa: E402
import markdup_cases as mc  # noqa: E402
import sort_bam_cases as sc  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "bam_stage_digests.json")
NOT_COUNTS = ("bytes_in", "backend", "path")


def group_memory():
    """A --memory under which the sort fixture falls into at least three groups: its largest bucket's bytes"""
    b = sc.bam()
    memory = max(sc.bucket_bytes(b))
    assert sc.expected_groups(b, memory)[0] >= 3
    return memory


def entries():
    """[(name, tool, way, options)]"""
    out = []
    for way in sc.WAYS:
        out.append(("sort-%s-default" % way, "sort", way, {}))
        out.append(("sort-%s-groups" % way, "sort", way, dict(memory=group_memory())))
    for way in mc.WAYS:
        for remove in (False, True):
            out.append(("markdup-%s-%s" % (way, "remove" if remove else "flag"), "markdup", way, dict(remove=remove)))
    for way in ic.WAYS:
        out.append(("index-%s" % way, "index", way, {}))
    return out


NAMES = [e[0] for e in entries()]


def write_inputs(tmp):
    """-> {(tool, way): path}: the three fixtures in each of their block layouts"""
    paths = {}
    for tool, cases in (("sort", sc), ("markdup", mc), ("index", ic)):
        b = cases.bam()
        for way, kw in cases.WAYS.items():
            paths[tool, way] = os.path.join(str(tmp), "%s_%s.bam" % (tool, way))
            b.write(paths[tool, way], index=False, **kw)
    return paths


def run(name, inputs, out_fn, backend="host", deflate="host", **how):
    """The entry `name` run into out_fn -> dict(sha256 of the whole file, counts)"""
    from clair_amd import index_bam, markdup_bam, sort_bam
    _, tool, way, options = entries()[NAMES.index(name)]
    if tool == "index":
        result = index_bam.build_index(inputs[tool, way], out_fn, backend=backend, **how)
    else:
        call = sort_bam.sort_bam if tool == "sort" else markdup_bam.markdup_bam
        result = call(inputs[tool, way], out_fn, backend=backend, deflate=deflate, **dict(options, **how))
    with open(out_fn, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()
    return dict(sha256=digest, counts={k: v for k, v in result.items() if k not in NOT_COUNTS})


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        inputs = write_inputs(tmp)
        recorded = {name: run(name, inputs, os.path.join(tmp, name + ".out")) for name in NAMES}
    with open(GOLDEN, "w") as f:
        json.dump(recorded, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d entries" % (GOLDEN, len(recorded)))
