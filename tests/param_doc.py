"""The runtime parameters as include/summa_gpu.h documents them (test infrastructure): one comment line per parameter,
`"name"  range, default D: meaning`, in the block above sg_set_param."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def documented_defaults() -> dict:
    """{name: documented default} of every parameter the header lists"""
    hdr = open(os.path.join(ROOT, "include", "summa_gpu.h")).read()
    block = hdr[hdr.index("/* Runtime parameters."):hdr.index("int sg_set_param(")]
    return {m[1]: int(m[2]) for m in re.finditer(r'^ \*   "([a-z0-9_.]+)" +[^\n]*?, default (\d+):', block, flags=re.M)}


def table_names() -> set:
    """the names of the rows of the library's parameter table (kParams in csrc/summa_gpu.hip)"""
    src = open(os.path.join(ROOT, "circuits_halo2_amd", "csrc", "summa_gpu.hip")).read()
    table = src[src.index("constexpr ParamRow kParams[] = {"):src.index("#undef MSM_ROW")]
    return (set(re.findall(r'\{"([a-z0-9_.]+)", Scope::', table))
            | {"msm." + f for f in re.findall(r"\bMSM_ROW\((\w+),", table)}
            | {"ntt." + f for f in re.findall(r"\bNTT_ROW\((\w+),", table)})
