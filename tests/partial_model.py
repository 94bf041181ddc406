"""A byte-at-a-time Python restatement of the partial mode of decode_seq.hpp (template parameter PARTIAL of decode_seq_body:
LZ4_decompress_safe_partial, cbits/lz4.c:2179-2185, without a dictionary), loop for loop and rule for rule, so that the
kernel's rules can be held to the reference without a GPU: tests/test_partial_decode_host.py runs it over the fixture, and

    python tests/partial_model.py [N]

compares it with a live reference (oracle/_ref) on N random cases -- inputs of 0 .. 4096 bytes, 0-3 mutated bytes, targets
and capacities around every edge -- and prints how many differ.  Cases the reference itself answers differently over a buffer
of 0x00 and of 0xEE are counted apart.  What may differ: a match with offset 0 that the output end clips copies every byte
onto itself (:2112-2113), so the reference's bytes there are what one of its wide copies left in the buffer."""
import os
import random
import sys


def model(src, target, cap, fill=0):
    """(result, the first max(result, 0) bytes) of a partial decode of block src over a buffer pre-filled with `fill`"""
    E=min(target,cap)
    if target<0: return None
    iend=len(src); oend=E
    dst=bytearray([fill])*(E+64)
    buf=src+bytes(64)
    def rd(p): return buf[p] if 0<=p<len(buf) else 0
    if E==0: return 0,b''
    if iend==0: return -1,b''
    fast = E>=64
    ip=0;op=0
    def cpm(op,match,ml,offset):
        if offset==0:
            for j in range(ml): dst[op+j]=0
        else:
            for j in range(ml): dst[op+j]=dst[match+j]
    while True:
        token=rd(ip);ip+=1
        ll=token>>4
        state=None
        if fast:
            if ll==15:
                if ip>=iend-15: return -ip-1,b''
                acc=0
                while True:
                    s=rd(ip);ip+=1;acc+=s
                    if not(s==255 and ip<iend-15):break
                ll+=acc
                if op+ll>oend-32 or ip+ll>iend-32: fast=False; state='slc'
            else:
                if ip>iend-17: fast=False; state='slc'
            if state is None:
                dst[op:op+ll]=buf[ip:ip+ll]; ip+=ll;op+=ll
                offset=rd(ip)|(rd(ip+1)<<8);ip+=2
                match=op-offset
                ml=token&15
                if ml==15:
                    if match<0: return -ip-1,b''
                    acc=0
                    while True:
                        s=rd(ip);ip+=1;acc+=s
                        if ip>=iend-4: return -ip-1,b''
                        if s!=255:break
                    ml+=acc+4
                    if op+ml>=oend-64: fast=False; state='smc'
                else:
                    ml+=4
                    if op+ml>=oend-64: fast=False; state='smc'
                if state is None:
                    if match<0: return -ip-1,b''
                    cpm(op,match,ml,offset); op+=ml
                    continue
        if state is None:
            if ll!=15 and ip<iend-16 and op<=oend-32:
                dst[op:op+ll]=buf[ip:ip+ll]; op+=ll;ip+=ll
                ml=token&15
                offset=rd(ip)|(rd(ip+1)<<8);ip+=2
                match=op-offset
                if ml!=15 and offset>=8 and match>=0:
                    cpm(op,match,ml+4,offset);op+=ml+4;continue
                state='cm'
            else:
                if ll==15:
                    if ip>=iend-15: return -ip-1,b''
                    acc=0
                    while True:
                        s=rd(ip);ip+=1;acc+=s
                        if not(s==255 and ip<iend-15):break
                    ll+=acc
                state='slc'
        if state=='slc':
            if op+ll>oend-12 or ip+ll>iend-8:
                if ip+ll>iend: ll=iend-ip
                if op+ll>oend: ll=oend-op
                dst[op:op+ll]=buf[ip:ip+ll]; ip+=ll;op+=ll
                if op==oend or ip>=iend-2: break
            else:
                dst[op:op+ll]=buf[ip:ip+ll]; ip+=ll;op+=ll
            offset=rd(ip)|(rd(ip+1)<<8);ip+=2
            match=op-offset
            ml=token&15
            state='cm'
        if state=='cm':
            if ml==15:
                acc=0
                while True:
                    s=rd(ip);ip+=1;acc+=s
                    if ip>=iend-4: return -ip-1,b''
                    if s!=255:break
                ml+=acc
            ml+=4
            state='smc'
        # smc
        if match<0: return -ip-1,b''
        if op+ml>oend-12:
            mlen=min(ml,oend-op)
            if offset!=0: cpm(op,match,mlen,offset)
            op+=mlen
            if op==oend: break
            continue
        cpm(op,match,ml,offset); op+=ml
    assert all(b==fill for b in dst[E:])
    return op,bytes(dst[:op])


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_partial_golden as G
    L = G.load_reference()
    rnd = random.Random(5)
    bad = tot = dep = 0
    for trial in range(int(sys.argv[1]) if len(sys.argv) > 1 else 20000):
        n = rnd.choice((0, 1, 12, 13, 64, 300, 1500, 4096))
        data = G.text_like(n, trial) if rnd.random() < 0.8 else bytes(rnd.randrange(256) for _ in range(n))
        block = bytearray(G.ref_compress(L, data)) if n else bytearray(b"\0")
        for _ in range(rnd.randint(0, 3)):
            block[rnd.randrange(len(block))] = rnd.randrange(256)
        block = bytes(block)
        target = rnd.randint(0, n + 40)
        cap = rnd.choice((target, n, n + 64, max(target - 5, 0)))
        r0, r1 = G.ref_partial(L, block, target, cap, 0), G.ref_partial(L, block, target, cap, 0xEE)
        if r0 != r1:
            dep += 1
            continue
        tot += 1
        m = model(block, target, cap, 0xEE)
        if (m[0], m[1] if m[0] >= 0 else b"") != r0:
            bad += 1
            print("differs: n %d block %s target %d cap %d: reference %d, model %d" % (n, block.hex(), target, cap, r0[0], m[0]))
    print("cases %d, model differs %d, dropped (depend on the buffer) %d" % (tot, bad, dep))


if __name__ == "__main__":
    main()
