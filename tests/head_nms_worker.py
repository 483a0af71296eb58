"""Child process of head_cases.check_nms_row_scan_child: runs the NMS cases in a process that was started with
CFUN_NMS_SCAN_LDS=0 (the library reads the knob once per process) and writes the keep lists to an .npz file.
usage: head_nms_worker.py <device> <out.npz>"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

if __name__ == "__main__":
    import head_cases as hc
    hc.nms_worker_main(sys.argv[1], sys.argv[2])
