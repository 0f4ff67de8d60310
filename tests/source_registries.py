"""TEST INFRASTRUCTURE - the constants that the kernels' sources define ONCE, parsed from where they are defined: the Philox stream
words (the enum of ``csrc/pf_philox.hpp``) and the launch-trace entry codes (the enum of ``csrc/pf_host.hpp``).  A definition
anywhere else under ``csrc/`` fails the parse: the tests that compare these with their own tables (``philox_ref.STREAMS``,
``theta_oracle.JITTER_STREAM``, ``smoothing_mh_oracle.PHILOX_STREAM``, ``ops.TRACE_ENTRY``) then see every word there is."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyfilter_amd", "csrc")
_NUMBER = r"(0[xX][0-9a-fA-F]+|\d+)u?"


def _one_enum(prefix, home, skip=()):
    """``{name without prefix: value}`` of the one enum in ``home`` that defines ``prefix*`` names (decimal or hexadecimal)."""
    defines = rf"#\s*define\s+{prefix}\w+|{prefix}\w+\s*=(?!=)"
    found = {}
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        sites = [s for s in re.findall(defines, text) if not any(k in s for k in skip)]
        if name != home:
            assert not sites, f"{name} defines {sites}: {home} holds every {prefix}*"
            continue
        bodies = re.findall(rf"enum\s*(?::\s*\w+\s*)?\{{([^}}]*{prefix}[^}}]*)\}}", text)
        assert len(bodies) == 1, bodies
        pairs = re.findall(rf"{prefix}(\w+)\s*=\s*{_NUMBER}", bodies[0])
        assert len(pairs) == len(sites), f"a {prefix}* outside the enum of {home}, or a value the parser does not read"
        for key, val in pairs:
            assert key not in found, f"{prefix}{key} defined twice"
            found[key] = int(val, 0)
    return found


def streams_in_sources():
    return _one_enum("PF_STREAM_", "pf_philox.hpp")


def trace_codes_in_sources():
    return _one_enum("PF_TRACE_", "pf_host.hpp", skip=("PF_TRACE_LEN", "PF_TRACE_FIELDS"))
