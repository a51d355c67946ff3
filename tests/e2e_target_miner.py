"""Target-aware CPU miner for tests/test_e2e_target.py: tests/e2e_oracle_miner.py's process (join
over LSP, Request -> scan -> Result) that answers a Request carrying a Target as mh_miner_handle
does -- with the chunk's first nonce whose hash is <= Target, else the chunk's minimum -- from the
test oracle (test infrastructure only; the product miner is bin/minehip-miner).

    python tests/e2e_target_miner.py HOST:PORT
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "bitcoin-miner_amd"), HERE]

import minehip  # noqa: E402
from minehip import lsp  # noqa: E402
from e2e_oracle_miner import params  # noqa: E402
from target_cases import chunk_answer  # noqa: E402


def main():
    cl, err = lsp.NewClient(sys.argv[1], params())
    if err is not None:
        print("Failed to join with server:", err)
        return 1
    cl.Write(minehip.marshal(minehip.NewJoin()))
    while True:
        payload, err = cl.Read()
        if err is not None:
            break
        m = minehip.unmarshal(payload)
        if m is None or m.Type != minehip.Request:
            continue
        cl.Write(minehip.marshal(minehip.NewResult(*chunk_answer(m.Data, m.Lower, m.Upper, m.Target))))
    cl.Close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
