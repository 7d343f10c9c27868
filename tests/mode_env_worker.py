"""Child process of tests/test_mode_threads.py: loads libmms_hip.so (no GPU is touched) and prints what
mms_get_euclid_backward_mode() reports on the main thread and on a new thread, one "<where> <mode>" line each.
`--main-sets V`: the main thread first calls mms_set_euclid_backward_mode(V), before anything read the mode."""
import ctypes
import os
import sys
import threading

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mms_answer_selection_amd", "libmms_hip.so")


def main(argv):
    lib = ctypes.CDLL(LIB)
    if "--main-sets" in argv:
        assert lib.mms_set_euclid_backward_mode(int(argv[argv.index("--main-sets") + 1])) == 0
    print("main", lib.mms_get_euclid_backward_mode())
    seen = []
    t = threading.Thread(target=lambda: seen.append(lib.mms_get_euclid_backward_mode()))
    t.start()
    t.join()
    print("thread", seen[0])


if __name__ == "__main__":
    main(sys.argv[1:])
