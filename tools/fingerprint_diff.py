"""Did two runs compute the same bits?  Compares two RUN_DIR/fingerprints.jsonl files (rspnet_amd/fingerprint.py; written with the
config key "fingerprint"): the first global step at which the gradient or the state fingerprints differ and the tensors involved
(exit status 1), or "identical over N records" (exit status 0).  Headers that disagree -- the runs fingerprinted different lists of
tensors -- are an error (exit status 2).

    python3 tools/fingerprint_diff.py A/fingerprints.jsonl B/fingerprints.jsonl"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    if len(argv) != 2:
        print(__doc__, file=sys.stderr)
        return 2
    from rspnet_amd import fingerprint as F
    try:
        diff = F.first_difference(argv[0], argv[1])
        n = min(len(F.load_file(argv[0])[1]), len(F.load_file(argv[1])[1]))
    except (ValueError, OSError) as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    if diff is None:
        print(f"identical over {n} records")
        return 0
    i, gs, sides = diff
    print(f"first difference at global_step {gs} (record {i}):")
    for side, names in sides.items():
        print(f"  {side}: {len(names)} tensors differ: {', '.join(names[:12])}{', ...' if len(names) > 12 else ''}")
    return 1


if __name__ == "__main__":
    sys.exit(main())
