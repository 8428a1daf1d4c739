#!/usr/bin/env python3
"""Run a module as __main__ with Python's random draws preset to one value (tools/make_train_set_goldens.py):

    python tools/run_with_fixed_random.py VALUE MODULE [arguments of the module]

random.uniform(a, b) and random.random() both return VALUE, so that a script which thins its output by `uniform(0, 1) <= p` or
`random() < r` keeps exactly the items whose probability admits VALUE: its rule can be minted into a golden file without its stream.
"""
import random
import runpy
import sys

value, module = float(sys.argv[1]), sys.argv[2]
random.uniform = lambda a, b: value
random.random = lambda: value
sys.argv = [module] + sys.argv[3:]
runpy.run_module(module, run_name="__main__", alter_sys=True)
