"""Records tests/golden/dropin_contract.json: what tests/_dropin_contract.py produces, case by
case, with the package as it stands (needs the GPU and the built library).  The file was
recorded with the package as it was BEFORE the drop-ins were merged onto chocosgd_amd/wire.py
and is the acceptance of that change: it is not re-recorded to make a change pass.

Usage:  python tests/golden/gen_dropin_contract.py [--out FILE] [--stable-against FILE]

--stable-against FILE (a file an earlier run, in another process, wrote with --out): every
top-k and random-k case must be identical in the two runs; a hash of a sign or QSGD case that
differs between them is left out of the file written (the case stays) and printed.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import pytest  # noqa: E402

import _dropin_contract as C  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "dropin_contract.json"))
    ap.add_argument("--stable-against")
    args = ap.parse_args()
    names = C.traced_names()
    cases = {}
    for name in C.NAMES:
        with pytest.MonkeyPatch.context() as mp:
            cases[name] = C.run_case(name, mp, names)
    record = json.loads(json.dumps({"traced": names, "cases": cases}))
    if args.stable_against:
        with open(args.stable_against) as f:
            other = json.load(f)
        assert other["traced"] == record["traced"]
        for name, mine in record["cases"].items():
            theirs = other["cases"][name]
            for key in [k for k, v in mine["hashes"].items() if theirs["hashes"].get(k) != v]:
                assert "top_k" not in name and "random_k" not in name, f"{name}: {key} differs between two runs"
                print(f"unstable, left out: {name} {key}")
                del mine["hashes"][key], theirs["hashes"][key]
            assert mine == theirs, f"{name}: two runs differ beyond their hashes"
    with open(args.out, "w") as f:  # one case per line
        lines = ['"{}": {}'.format(name, json.dumps(case, sort_keys=True)) for name, case in record["cases"].items()]
        f.write('{{"traced": {},\n"cases": {{\n{}\n}}}}\n'.format(json.dumps(record["traced"]), ",\n".join(lines)))
    print(f"wrote {args.out}: {len(cases)} cases")


if __name__ == "__main__":
    main()
