# same-box A/B of the host-fed measurement's knobs (copy streams the batch is cut over, batches uploaded ahead)
f=$(mktemp)
for e in "TDEED_FEED_STREAMS=1" "TDEED_FEED_STREAMS=1 TDEED_FEED_AHEAD=3" "TDEED_FEED_STREAMS=1 TDEED_FEED_AHEAD=4" "TDEED_FEED_STREAMS=1 TDEED_FEED_AHEAD=1"; do
  env $e python bench.py --full --no-train --no-cpu-baseline > $f 2>/dev/null
  python -c "
import json; d=json.loads(open('$f').read().strip().splitlines()[-1]); f=d['fed_from_host']; print('[$e]', d['value'], f['value'], f['h2d_GBps'], f['frac_of_resident'])"
done
