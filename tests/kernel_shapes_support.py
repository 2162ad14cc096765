"""tests/tools/check_kernel_shapes.cpp for the tests that use it: the host program over csrc/dn_shapes.h, built with the host compiler
and run as its own process."""
import host_program_support


def build_program(directory, sanitize=False):
    return host_program_support.build("check_kernel_shapes", directory, sanitize=sanitize)


def run_program(exe, **keys):
    """Without keys: the walk's {"cases", "digest", "bad"}.  With keys (num_cus, num_envs, configuration fields): {"fused", "single"}."""
    return host_program_support.run(exe, *["%s=%s" % kv for kv in keys.items()], timeout=120)
