"""Generates tests/golden/png_encode_pins.json: the SHA-256 and the length of the file image_writer.encode_png gives for every case of
tests/png_encode_cases.py, through the host emulator -- the very runs tests/test_png_encode_host.py performs, group by group.

    python tests/golden/make_png_encode_pins.py <what the bytes come from: a commit>

The encoder's arithmetic is integer-only and every tie is broken by an index, so the emulator's bytes are the device's bytes:
tests/test_png_encode_{host,gpu}.py hold both to these pins.  The committed file was written at 9ddf48a ("Add HIP PNG decoder"), the
commit BEFORE the encoder and the decoder came to share csrc/png_common.h: it pins what the encoder wrote before that change.  Run
it again only where the encoder's bytes are meant to change, and say so in the commit.
"""
import hashlib
import json
import os
import sys
import tempfile
from pathlib import Path

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.join(TESTS, "hipemu"))

import host_child  # noqa: E402
import png_encode_cases as K  # noqa: E402

OUT = os.path.join(HERE, "png_encode_pins.json")


def main(source):
    pins = {}
    with tempfile.TemporaryDirectory(prefix="png-pins-") as tmp:
        for names in K.GROUPS:
            res = host_child.run_child(os.path.join(TESTS, "test_png_encode_host.py"), "cases:" + ",".join(names), Path(tmp), timeout=600)
            for n in names:
                png = res["png_" + n].tobytes()
                pins[n] = {"sha256": hashlib.sha256(png).hexdigest(), "bytes": len(png)}
    assert sorted(pins) == sorted(K.CASES)
    with open(OUT, "w") as fh:
        json.dump({"source": source, "through": "tests/hipemu (host emulator)", "cases": {n: pins[n] for n in K.CASES}}, fh, indent=1)
        fh.write("\n")
    print("wrote %s: %d cases" % (OUT, len(pins)))


if __name__ == "__main__":
    main(sys.argv[1])
