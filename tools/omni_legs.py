import os, sys, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
pkg = bench.load_pkg(); be = pkg.backend(0)
print(json.dumps(bench.omni_module_legs(pkg, be)))
