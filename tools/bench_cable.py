#!/usr/bin/env python3
"""Times the cable (radial profile) adjoint for 4M rays x ~512 steps with rays in random order and in source-pixel
order (neighbouring rays at nearly the same radius -> same-bin LDS adds, the case the pair / quad pre-reduction
of k_backtrace_cable is for).  Two JSON lines.

    python tools/bench_cable.py opl [OUT.json]

times, at the same sizes and for both orders, trace_cable_opl against trace_cable, and backtrace_cable_opl (profile only,
rays only, both) against backtrace_cable and backtrace_cable_rays: the calls alternate in one session, every figure is the
median of 7 single calls between device events.  One JSON line, also written to OUT.json.

    python tools/bench_cable.py field [OUT.json]

times, the same way, trace_cable_field against trace_cable_opl, and backtrace_cable_field (profile only, field only, both
profile gradients, rays only, everything) against backtrace_cable_opl (profile only, rays only, both); the second profile
is a group index N_g = n + 0.5 (n - n_cladding).  `ratios`: the forward to trace_cable_opl; the adjoint's profile-only,
field-only and both-gradients runs to backtrace_cable_opl's profile-only run, rays only to its rays-only run, everything to
its run with both outputs."""
import sys, json, torch, numpy as np
sys.path.insert(0,'.')
from adjointnonlinearraytracing_amd import drrt
drrt.options.check_failed=False
dev=torch.device('cuda:0')
rres, radius = 257, 1.0
ds = radius/(rres-1)/2; length = 512*ds
prof = torch.sqrt(2.0 - torch.linspace(0,1,rres)**2).to(dev)
n=2048*2048
g=torch.Generator(device=dev).manual_seed(0)
ang=torch.rand(n,device=dev,generator=g)*6.2831853; rad=0.9*radius*torch.sqrt(torch.rand(n,device=dev,generator=g))
pos=torch.stack([radius+rad*torch.cos(ang), torch.full((n,),0.37*ds,device=dev), radius+rad*torch.sin(ang)],-1)
vel=torch.randn(n,3,device=dev,generator=g)*0.05; vel[:,1]=1; vel/=vel.norm(dim=1,keepdim=True)
tg=torch.tensor([[radius,0.75*length,radius]],device=dev).expand(n,3).contiguous()
T=drrt.TracerC()
xt,vt,d2=T.trace_cable(prof,radius,length,pos,vel,tg,ds)
one=torch.ones_like(xt)
def timed(fn,reps=5):
    fn(); torch.cuda.synchronize()
    a,b=torch.cuda.Event(enable_timing=True),torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize(); return a.elapsed_time(b)/reps
mode=sys.argv[1] if len(sys.argv)>1 else 'adjoint'
if mode=='adjoint': print(json.dumps(dict(adj_random_order_ms=timed(lambda: T.backtrace_cable(prof,radius,length,xt,vt,one,one,ds)))))
# pixel-ordered source (neighbouring rays at nearly the same radius)
side=2048
i=torch.arange(side,device=dev,dtype=torch.float32)
X,Z=torch.meshgrid(i,i,indexing='ij')
px=(X.flatten()+0.5)/side*2*radius; pz=(Z.flatten()+0.5)/side*2*radius
pos2=torch.stack([px, torch.full((n,),0.37*ds,device=dev), pz],-1)
vel2=torch.zeros(n,3,device=dev); vel2[:,1]=1
xt2,vt2,_=T.trace_cable(prof,radius,length,pos2,vel2,tg,ds)
if mode=='adjoint': print(json.dumps(dict(adj_pixel_order_ms=timed(lambda: T.backtrace_cable(prof,radius,length,xt2,vt2,one,one,ds)))))

def opl_times(pos,vel):
    """{call: median ms of 7}, the calls taken in turn 7 times over."""
    xt,vt,_,opl,rec=T.trace_cable_opl(prof,radius,length,pos,vel,tg,ds)
    dopl=torch.ones_like(opl)
    calls=dict(
        trace_cable=lambda: T.trace_cable(prof,radius,length,pos,vel,tg,ds),
        trace_cable_opl=lambda: T.trace_cable_opl(prof,radius,length,pos,vel,tg,ds),
        backtrace_cable=lambda: T.backtrace_cable(prof,radius,length,xt,vt,one,one,ds),
        backtrace_cable_rays=lambda: T.backtrace_cable_rays(prof,radius,length,pos,vel,tg,one,one,ds),
        backtrace_cable_opl_profile=lambda: T.backtrace_cable_opl(prof,radius,length,pos,xt,vt,rec,one,one,dopl,ds,rays=False),
        backtrace_cable_opl_rays=lambda: T.backtrace_cable_opl(prof,radius,length,pos,xt,vt,rec,one,one,dopl,ds,profile=False),
        backtrace_cable_opl_both=lambda: T.backtrace_cable_opl(prof,radius,length,pos,xt,vt,rec,one,one,dopl,ds))
    for fn in calls.values(): fn()
    torch.cuda.synchronize()
    ms={k:[] for k in calls}
    for _ in range(7):
        for k,fn in calls.items():
            a,b=torch.cuda.Event(enable_timing=True),torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); torch.cuda.synchronize(); ms[k].append(a.elapsed_time(b))
    out={k:float(np.median(v)) for k,v in ms.items()}
    out['backtrace_cable_plus_rays']=out['backtrace_cable']+out['backtrace_cable_rays']
    out['mean_record_iteration']=float(rec.float().mean())
    return out
if mode=='opl':
    res=dict(rays=n,rres=rres,random_order_ms=opl_times(pos,vel),pixel_order_ms=opl_times(pos2,vel2))
    print(json.dumps(res))
    if len(sys.argv)>2: json.dump(res,open(sys.argv[2],'w'),indent=1)

def field_times(pos,vel):
    """{call: median ms of 7}, the calls taken in turn 7 times over, and the ratios to the OPL pair."""
    fld=prof+0.5*(prof-prof[-1])
    xt,vt,_,tau,rec=T.trace_cable_field(prof,fld,radius,length,pos,vel,tg,ds)
    dtau=torch.ones_like(tau)
    bo=lambda **kw: (lambda: T.backtrace_cable_opl(prof,radius,length,pos,xt,vt,rec,one,one,dtau,ds,**kw))
    bf=lambda r,f,y: (lambda: T.backtrace_cable_field(prof,fld,radius,length,pos,xt,vt,rec,one,one,dtau,ds,r,f,y))
    calls=dict(
        trace_cable_opl=lambda: T.trace_cable_opl(prof,radius,length,pos,vel,tg,ds),
        trace_cable_field=lambda: T.trace_cable_field(prof,fld,radius,length,pos,vel,tg,ds),
        backtrace_cable_opl_profile=bo(rays=False), backtrace_cable_opl_rays=bo(profile=False), backtrace_cable_opl_both=bo(),
        backtrace_cable_field_profile=bf(True,False,False), backtrace_cable_field_field=bf(False,True,False),
        backtrace_cable_field_both_profiles=bf(True,True,False), backtrace_cable_field_rays=bf(False,False,True),
        backtrace_cable_field_everything=bf(True,True,True))
    for fn in calls.values(): fn()
    torch.cuda.synchronize()
    ms={k:[] for k in calls}
    for _ in range(7):
        for k,fn in calls.items():
            a,b=torch.cuda.Event(enable_timing=True),torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); torch.cuda.synchronize(); ms[k].append(a.elapsed_time(b))
    out={k:float(np.median(v)) for k,v in ms.items()}
    out['ratios']=dict(
        forward=out['trace_cable_field']/out['trace_cable_opl'],
        profile=out['backtrace_cable_field_profile']/out['backtrace_cable_opl_profile'],
        field=out['backtrace_cable_field_field']/out['backtrace_cable_opl_profile'],
        both_profiles=out['backtrace_cable_field_both_profiles']/out['backtrace_cable_opl_profile'],
        rays=out['backtrace_cable_field_rays']/out['backtrace_cable_opl_rays'],
        everything=out['backtrace_cable_field_everything']/out['backtrace_cable_opl_both'])
    out['mean_record_iteration']=float(rec.float().mean())
    return out
if mode=='field':
    res=dict(rays=n,rres=rres,random_order_ms=field_times(pos,vel),pixel_order_ms=field_times(pos2,vel2))
    print(json.dumps(res))
    if len(sys.argv)>2: json.dump(res,open(sys.argv[2],'w'),indent=1)
