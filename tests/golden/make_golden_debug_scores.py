"""Writes tests/golden/debug_scores.json: the vector of the reference's own test of debugScores
(pkg/scheduler/frameworkext/debug_test.go:91-176 TestDebugScores), transcribed as data: the pod, topN, the four
feasible nodes in order, the ten plugins' weighted scores per node, and the expected RenderMarkdown text byte for
byte. Run from the repo root: python tests/golden/make_golden_debug_scores.py"""
import json
import os

NODES = ["cn-hangzhou.10.0.4.50", "cn-hangzhou.10.0.4.51", "cn-hangzhou.10.0.4.19", "cn-hangzhou.10.0.4.18"]
POD = "default/curlimage-545745d8f8-rngp7"

# debug_test.go:92-153, in the order of the map literal; scores in the order of NODES
PLUGINS = {
    "ImageLocality": [0, 0, 0, 0],
    "InterPodAffinity": [0, 0, 0, 0],
    "LoadAwareScheduling": [85, 87, 55, 15],
    "NodeAffinity": [0, 0, 0, 0],
    "NodeNUMAResource": [0, 0, 0, 0],
    "NodeResourcesBalancedAllocation": [96, 96, 95, 90],
    "NodeResourcesFit": [93, 94, 91, 82],
    "PodTopologySpread": [200, 200, 200, 200],
    "Reservation": [0, 0, 0, 0],
    "TaintToleration": [100, 100, 100, 100],
}

HEADER = ["#", "Pod", "Node", "Score"] + sorted(PLUGINS)
# debug_test.go:169-174: (rank, node, total, the plugin columns)
ROWS = [
    [0, "cn-hangzhou.10.0.4.51", 577, 0, 0, 87, 0, 0, 96, 94, 200, 0, 100],
    [1, "cn-hangzhou.10.0.4.50", 574, 0, 0, 85, 0, 0, 96, 93, 200, 0, 100],
    [2, "cn-hangzhou.10.0.4.19", 541, 0, 0, 55, 0, 0, 95, 91, 200, 0, 100],
    [3, "cn-hangzhou.10.0.4.18", 487, 0, 0, 15, 0, 0, 90, 82, 200, 0, 100],
]


def expected() -> str:
    lines = ["| " + " | ".join(HEADER) + " |",
             "| --- | --- | --- |" + " ---:|" * (len(HEADER) - 3)]
    for r in ROWS:
        lines.append("| " + " | ".join(str(x) for x in [r[0], POD, *r[1:]]) + " |")
    return "\n".join(lines)


G = {"source": "pkg/scheduler/frameworkext/debug_test.go:91-176 TestDebugScores", "topn": 4, "pod": POD,
     "nodes": NODES, "plugins": PLUGINS, "expected": expected()}

if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "debug_scores.json")
    with open(path, "w") as f:
        json.dump(G, f, indent=1)
        f.write("\n")
    print(path)
