"""The device's own chain over tests/links_cases.py's construction, ending in close_gaps: index_contigs -> align_reads ->
align_gapped -> pair_inserts -> ctg_links -> scaffolds -> close_gaps.  The result is the genome, and it is the model's on the
device's own intermediate outputs.  A file of its own: what fails here and not in tests/test_gpu_close_gaps.py (whose
inputs come from the models) lies in a step in front of kc_close_gaps."""
import numpy as np
import pytest

import close_model as M
import links_cases as LC
import mhm2_kmer_analysis_v2_amd as pkg
import scaffold_model as SM
from test_gpu_gap_align import block_arrays, read_arrays

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(LC.LAYOUTS))
def test_the_devices_own_chain_closes_the_construction_to_the_genome(name):
    import torch
    layout, gaps = LC.LAYOUTS[name]
    G = LC.genome(19)
    contigs = LC.contigs_of(G, layout)
    reads, places = LC.pairs_of(G, 19)
    b, o = read_arrays(reads)
    kw = dict(end_slack=0, max_overlap=50, max_splint_gap=50)
    with pkg.KmerCounter(LC.K) as kc:
        kc.index_contigs(*block_arrays(contigs))
        alns, _, _ = kc.align_reads(b, o)
        gapped, _ = kc.align_gapped(b, o, alns)
        _, pairs, _ = kc.pair_inserts(o, gapped, max_insert=1000)
        links, _, lst, _ = kc.ctg_links(o, gapped, pairs, insert_avg=LC.FRAGMENT, max_insert=1000, **kw)
        _, _, scafs, members, sst = kc.scaffolds(links)
        assert sst["scaffolds"] == 1 and SM.scaffold(contigs, links.view(SM.LINK_DTYPE))[3].tobytes() == members.tobytes()
        res = kc.close_gaps(b, o, gapped, scafs, members, **kw)
        want = M.close_gaps(contigs, reads, gapped, scafs.view(SM.SCAFFOLD_DTYPE), members.view(SM.MEMBER_DTYPE), **kw)
        assert [x.tobytes() for x in res[:5]] == [want[0]] + [x.tobytes() for x in want[1:5]] and res[5] == want[5]
        assert kc.close_gaps_strings(b, o, gapped, scafs, members, **kw) == [G]
        st = res[5]
        assert st["n_bases_left"] == 0 and st["filled"] == st["gaps"] == (2 if name == "gaps" else 1) and st["cands"] == lst["splint_cands"]
        # device tensors all the way give the same bytes, and the closed block is a contig block
        dev = [torch.from_numpy(np.frombuffer(x.tobytes(), dtype=np.int64 if i == 1 else np.uint8).copy()).cuda()
               for i, x in enumerate((b, o, gapped, scafs, members))]
        on = kc.close_gaps(*dev, **kw)
        assert [x.cpu().numpy().tobytes() for x in on[:5]] == [x.tobytes() for x in res[:5]] and on[5] == st
        kc.index_contigs(on[0], on[1])
        assert kc.contig_index_info() == (len(G) + 1, 1)
